// dindel_gpu — the --analysis indels --doDiploid window loop on the GPU likelihood path:
//   (BAM + .bai, window file, reference FASTA | haplotype file[, library file])  ->  PREFIX.glf.txt
//
// Restates DetInDel::detectIndels (reference DInDel.cpp:1265-1424) as prepare-N / compute / reduce-N:
//   prepare  per window, in file order: getReads (get_reads.cpp) and the window's candidate haplotypes.  With --ref FASTA they are BUILT
//            here as the reference builds them (getHaplotypes, DInDel.cpp:1526-1645), for all windows of a batch at once from the reads just
//            selected: the block tables of the empirical distribution and the alignment to the reference on the device
//            (getHaplotypesBatch, alignHaplotypesBatch: one launch each per batch), the variants of every alignment by the variants
//            kernel behind it (--hostConvert: on the host), then the maxHapReadProd check of :395-399.  What getHaplotypes throws becomes
//            the window's skipped line and a late skip (below); where it returns `true` (:1569, :1581) the window writes no line.
//            With --hapFile they are read from a haplotype file instead (window_io.hpp), and --ref has no effect;
//   compute  LikelihoodEngine::computeLikelihoodsBatch over the N prepared windows (one launch sequence on the GPU);
//   reduce   per window: diploidGLF (diploid_glf.cpp) -> the window's lines, or the skipped-window line with the message the
//            reference would print ("error_" + what was thrown); lines are written in file order.
// The stages run as a pipeline: the main thread reads the window file and cuts it into batches; --prepareThreads workers, each
// with its own handle on the BAM file and its own read buffer, prepare whole batches side by side; one thread feeds the GPU in
// batch order; one thread (with --reduceThreads helpers, each window into its own buffer) reduces and writes in window order.
// --bamFiles LIST (one path per line, first word of the line; reference DInDel.cpp:64-88): the files are pools of one read buffer
// (Read::fetchFuncVectorPooled, poolID = position in the list).  With several pools the buffer's ORDER depends on its history — a
// window's new records are appended pool after pool behind the survivors of the windows before — and std::sort's order inside a tie of
// mapping qualities follows it, so a worker does not start a batch with an empty buffer: it first replays read selection over the
// batch's look-back (the preceding windows of the chromosome back to one whose reads have all left the buffer by the batch's first
// window), which leaves the buffer in the state the window-by-window loop would have.  What a worker cannot see is a window skipped
// AFTER read selection (an exception of the haplotype construction under --ref, of the likelihood or of the genotyping step: "hapblock",
// "Not enough blocks.", "hapSize error.", "Nan detected", ...): the reference empties
// the buffer after it (DInDel.cpp:1404-1405).  The writer sees it: from the window behind such a LATE skip it re-prepares, from an empty
// buffer and window by window, every window whose buffer could still hold a record of that moment (same chromosome, leftPos less than
// 2 maxInsert + 200 behind the first re-prepared window's rightPos) with a read fetcher, an engine and the reduce step of its own, and
// writes those results instead of the ones prepared ahead — beyond that reach both histories hold the same records in the same order.
// One BAM file: with a single pool the read buffer's reset (after a skipped window in the reference, DInDel.cpp:1401-1408; at
// the head of every batch here) does not change which reads a window sees — the buffer always holds the file's reads starting in
// [leftPos - maxInsert - 200, rightPos + maxInsert), in file order — so preparing windows ahead of their predecessors'
// likelihood step, and batches side by side, is exact.  (One counter does depend on the buffer's history: "Too many reads in
// region" fires on buffer size + records fetched > 100 * maxRead, which at a batch's first window is counted as after a reset.)
//
// Options (names follow the reference's CLI, DInDel.cpp:4079-4170):
//   --bamFile F | --bamFiles LIST   --varFile F [--varFileIsOneBased] --ref FASTA | --hapFile F   --outputFile PREFIX [--libFile F] [--faster] [--filterHaplotypes]
//   --ref mode only (the reference's names and defaults, DInDel.cpp:4127, :4132, :4139): [--maxHap N] [--skipMaxHap N] [--changeINStoN]
//                     [--hostDistribution] block tables on the host   [--hostConvert] alignments to variants on the host
//   [--maxRead N] [--maxReadLength N] [--minReadOverlap N] [--mapQualThreshold X] [--pError X] [--pMut X] [--maxLengthIndel N]
//   [--filterReadAux STR] [--flankRefSeq N] [--flankMaxMismatch N] [--priorSNP X] [--priorIndel X] [--capMapQualThreshold X] [--capMapQualFast X]
//   [--maxHapReadProd N] [--batchWindows N] [--prepareThreads N] [--computeThreads N] [--packThreads N] [--reduceThreads N] [--device D | --devices D0,D1,...] [--quiet]
//   [--outputRealignedBAM]   per window PREFIX.ra.INDEX_TID_LEFT_RIGHT.bam with the reads realigned through the most likely haplotype
//                     pair (DInDel.cpp:589-620; main model only, like the reference; the haplotype file needs its A records)
//   [--deviceCigars [--cigarOpsCap N]]  with --outputRealignedBAM: the reads' CIGARs are computed on the device from the alignments it keeps
//                     (at most N operations per read, default 8) and come back instead of the per-base alignments; a read with more
//                     operations is redone on the host from its window's alignments — the whole window is recomputed once for that, one
//                     window at a time, so a small N costs a recompute per affected window — (counted in the timing line).  The files are the
//                     same byte for byte.  The engines then merge as many batches per launch as without realigned BAMs.  No effect
//                     without --outputRealignedBAM (main model, like that option)
//   [--deviceRealign [--cigarOpsCap N]]  with --doPooled --outputRealignedBAM (and no --doDiploid): the device also picks the haplotype each read is
//                     realigned to (the pooled rule is compares alone, so its choice is the host's bit for bit) and only that pair's CIGAR comes
//                     back: 4 N + 16 bytes per READ instead of --deviceCigars' H (4 N + 12).  Reads over N operations are redone on the host as
//                     with --deviceCigars.  The files are the same byte for byte.  Refused with --doDiploid (the files that stay are then the
//                     diploid step's, whose haplotype pair the host computes after the batch has left the device) and with --faster; no
//                     effect without --outputRealignedBAM.  Wins over --deviceCigars
//   [--deviceRealignDiploid [--cigarOpsCap N]]  with --doDiploid --outputRealignedBAM: the diploid step's realigned reads from the device.  A kernel picks
//                     every window's MAP haplotype pair (maxLikelihoodPair's argmax) from the likelihoods in HBM and the prior table the prepare stage
//                     made, and certifies it: its sums are in another arithmetic than the host's, with a proven bound on the difference, so the pair is
//                     the host's whenever the best value leads the runner-up by more than the bound.  The realign launch follows on the same stream; one
//                     CIGAR per read comes back.  Windows that are not certified (ties, non-finite terms) are done on the host as without the switch and
//                     counted (pair_uncertified=).  The files are the same byte for byte.  Refused with --faster, without --doDiploid and together with
//                     --deviceRealign; no effect without --outputRealignedBAM; wins over --deviceCigars.  --checkDevicePair (tests): the reduce stage also
//                     runs maxLikelihoodPair on every certified window; pair_disagreements= must be 0 or the run fails
//   [--discover]      no --varFile: the run starts with the discovery stage (host/discover.hpp) on --devices[0] — candidate indels from the CIGARs
//                     of --bamFile (or, with --tid NAME --region A-B, of every file of --bamFiles), each realigned on the device, to
//                     PREFIX.variants.txt and PREFIX.libraries.txt exactly as `dindel_candidates --analysis getCIGARindels` writes them
//                     ([--batchCandidates N] [--eventsCap N] [--hostConvert] are that tool's), then the windows of python/makeWindows.py:129-207
//                     to PREFIX.windows.txt as `dindel_windows --oneFile` writes them ([--minDist N] [--minCount N] [--maxCount M]) —
//                     and the loop reads that file as if it had been given as --varFile.  Needs --ref; --hapFile beside it is an error.
//                     The stage is a barrier: windows are clusters of the whole candidate table.  The three files stay on disk.
//   [--useLibraries]  with --discover (whole-file run): PREFIX.libraries.txt is this run's --libFile; an explicit --libFile wins
//   [--candidateVCF F[,G...] [--minQual X] [--vcfCandidatesOnly]]  with --discover: known sites beside the sample's own candidates.
//                     The indels of the VCFs (plain or .gz; records with QUAL `.` or >= X, default 1) go to PREFIX.vcf.variants.txt exactly as
//                     `dindel_vcf2candidates` writes them (python/convertVCFToDindel.py:9-47; in a region run with that --tid / --region), are
//                     realigned on the device to PREFIX.vcf.realigned.variants.txt exactly as `dindel_candidates --analysis realignCandidates`
//                     writes them, and PREFIX.candidates.txt — what --minCount / --maxCount keep of PREFIX.variants.txt, then every known site
//                     (the filter never acts on them) — is what the windows are made from.  --vcfCandidatesOnly: no pass over the BAM's
//                     CIGARs, the known sites alone (--minCount / --maxCount / --useLibraries are errors then).  A conversion that fails
//                     stops the run before any window is prepared.
//   [--vcf F [--sampleID ID]]  after the loop PREFIX.glf.txt is converted to the VCF F as dindel_glf2vcf does with a list naming that one
//                     file (glf_to_vcf.hpp; python/mergeOutputDiploid.py:240-317); needs --ref
//   [--doPooled [--bayesa0 X] [--bayesType all|singlevariant|priorpersite]]  the pooled analysis (estimateHaplotypeFrequenciesBayesEM,
//                     DInDel.cpp:411-470, :2103-2930; host/pooled_em.hpp): per window one line per (candidate variant, pool).  Alone it writes
//                     only those lines; with --doDiploid both, the pooled lines of a window first; the likelihoods are computed once.  The
//                     compute stage builds the windows' active sets once a batch's results are back and runs all their EM slots in one launch
//                     (dd_pooled_em).  Defaults 0.001 and singlevariant.  With --outputRealignedBAM and no --doDiploid a window's file holds every
//                     read that lies on a haplotype realigned to the FIRST haplotype with the largest likelihood (DInDel.cpp:498-520; a note on
//                     stderr says so); with --doDiploid beside it the diploid step's file, which has the same name, is the one that stays.
//   [--pooledVcf F --numSamples N [--pooledGlf G]]  with --doPooled: after the loop PREFIX.glf.txt is converted to the VCF F as dindel_pooled2vcf
//                     does with a list naming that one file and --numBamFiles = the run's number of BAM files (host/pooled_vcf.hpp;
//                     python/mergeOutputPooled.py:202-575), then, with --pooledGlf, the per-pool likelihoods of the called sites go to G as
//                     dindel_pooled2glf writes them, the BAM names being the run's paths
//                     (python/makeGenotypeLikelihoodFilePooled.py:146-213).  Needs --ref.
//   [--timing]        one "timing:" line on stdout with the busy time of each stage
//   [--prepareOnly]   stop after the prepare stage (no likelihoods, no calls: profiling the read selection on a GPU-less host); with --ref
//                     in front of the haplotype stage, which needs the device
//   [--windowByWindow] tests: the writer re-does every window one after the other with a read buffer of its own (the reference's loop as it stands)
//   [--longWindows]   windows beyond the main kernels' limits (a haplotype > 766 bp, a read > 1024 bp, or with --maxLengthIndel >= 12 a
//                     haplotype > 574 bp) are computed by the long-window kernel (haplotypes up to 4,094 bp, reads up to 4,096 bp) instead
//                     of being written as skipped windows; no effect with --faster
//   [--longWindowsFaster]  the same for the --faster model (its own kernel): windows with a haplotype of 767..4,094 bp or a read of
//                     1,025..4,096 bp are computed instead of being written as skipped windows; effective only with --faster
//   [--wideDeletions]  --maxLengthIndel 32 and above (the reference takes any value): implies --longWindows, and every window within the
//                     long-window limits is then computed by that kernel's wide build (two bytes per back-pointer).  Required for such a value:
//                     without it the command is refused.  With --faster it only lifts the parameter check (that model compares the value
//                     with the haplotype length and does nothing else with it).  With --maxLengthIndel up to 31 it changes nothing but the
//                     implied --longWindows.  Refused with --audit / --auditFaster when --maxLengthIndel is 32 or more (the audit's shadow
//                     would be the same kernel).  At the default parameters such deletions are not on a read's most likely path anyway
//                     (DESIGN §27): the flag then changes which windows end with "hapSize error." and nothing else
//   [--audit N [--auditSeed S]]  main model: in every launch N of its ordinary windows (a seeded sample with every kernel build of the launch in
//                     it) are recomputed by the long-window kernel and compared on the device, bit for bit, with what the main kernels wrote
//                     (dd_compute_likelihoods_audit).  The output files are written as without the flag.  Every difference is printed to
//                     stderr (window line, tid, position, pair, field, both values); the timing line gains audit_windows=, audit_pairs= and
//                     audit_mismatches=; a run with any difference ends with exit status 3.  Refused with --faster (that model's long kernel
//                     shares its main kernel's text: no independent check); launches that ask for device CIGARs or realigned reads
//                     (--deviceCigars, --deviceRealign, --deviceRealignDiploid) take no audit
//   [--auditFaster N [--auditSeed S]]  --faster model, an option of its own as --longWindowsFaster is: in every launch N of the windows it
//                     computes (the long ones too with --longWindowsFaster; a seeded sample that holds the launch's longest ordinary
//                     haplotype and read) are recomputed by an independent shadow kernel, a second implementation of that model, and
//                     compared on the device, bit for bit, with what the --faster kernels wrote (dd_compute_likelihoods_faster_audit).
//                     Files, stderr lines, timing keys and exit status 3 as --audit's; also with --deviceIndelKeys.  Refused without --faster
//   [--deviceIndelKeys]  with --faster: the one number the window loop needs of a pair's per-base alignment under that model — the size of the
//                     record's indel map, DInDel.cpp:3529 — is counted on the device behind the likelihood launches and 2 bytes per pair come back
//                     instead of the alignment's 2 L; a pair with more than 64 distinct keys is recomputed on the host side with alignments
//                     (indel_key_fallbacks= in the timing line).  PREFIX.glf.txt is the same byte for byte.  The engines then merge as many
//                     batches per launch as the main model's.  No effect without --faster
//   [--mergeBatches N] batches already waiting when an engine becomes free ride in its launch, up to N (default 4; 2 when the per-base alignments come back)
//   [--computeAhead N] prepared batches that may wait for the GPU ahead of the next one to leave (default max(computeThreads + 1, prepareThreads))
//   tests and diagnostics only:
//   [--hostEM]        --doPooled: the EM slots run through dd_pooled_em_host on the CPU instead of on the device (the same bits)
//   [--noLookBack]    several pools: every batch starts with an empty read buffer (no replay of the windows in front of it)
//   [--injectLateSkip I,J,...]  the reduce step of these windows throws "hapSize error." (a late skip, also under --prepareOnly)
//   [--auditInject W] with --audit: one bit of the device copy of ll of window W's first pair (W: the window's line in the window file, from 1)
//                     is inverted in front of that window's audit and restored behind it, if the audit chose the window: the mismatch path
//                     without anything going wrong on the GPU (the output files are not affected)
//   [--lateSkipsKnown] the prepare stage is told of the injected late skips in advance and resets its buffers behind them
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <set>
#include <sstream>
#include <thread>
#include "batch_channels.hpp"
#include "compute_likelihoods.hpp"
#include "diploid_glf.hpp"
#include "discover.hpp"
#include "align_haplotypes.hpp"
#include "get_reads.hpp"
#include "glf_output.hpp"
#include "glf_to_vcf.hpp"
#include "haplotypes.hpp"
#include "pooled_em.hpp"
#include "pooled_vcf.hpp"
#include "python_text.hpp"
#include "realigned_bam.hpp"
#include "window_io.hpp"

using namespace dindel;

namespace {
struct WindowTask {
    int index; std::string tid; uint32_t pos, fileLeftPos, fileRightPos, leftPos, rightPos;
    AlignedCandidates candidates;
    std::vector<Read> reads;
    const std::vector<Haplotype> *haps;
    std::vector<Haplotype> built;        // --ref: the haplotypes made for this window in the run (haps points here); reused with the batch
    std::string message;                 // "ok" or the skipped message
    std::string note;                    // --ref: what getHaplotypes prints on cerr for this window; the writer prints it in window order
    bool skipped;
    bool passedOver;                     // --ref: getHaplotypes returned true (DInDel.cpp:1569 / :1581): no likelihoods, no line, not a skipped window
    bool lateSkip;                       // skipped by the likelihood or genotyping step, i.e. after read selection (DInDel.cpp:1369-1408)
    std::string lines;                   // what the reduce stage wrote for this window
    std::vector<double> pairPrior;       // --deviceRealignDiploid: getHaplotypePrior per haplotype pair (prepare stage), what the device's pair choice adds
    bool havePairPrior = false;
    long pairUncertified = 0, pairFallbackReads = 0, pairDisagreements = 0;   // ... of this window's last reduce step; the writer adds up what it writes
    bool computes() const { return !skipped && !passedOver; }    // the window reaches the likelihood step
    WindowJob job() const                // the window as the likelihood step takes it
    {
        WindowJob J;
        J.haps = haps; J.reads = &reads; J.leftPos = leftPos; J.rightPos = rightPos;
        if (havePairPrior) J.pairPrior = &pairPrior;
        return J;
    }
};
struct PooledJob { PooledWindow win; PooledPlan plan; };
struct Batch {
    long seq;                            // position in the file: batches are computed and written in this order
    // A finished batch goes back to the reader and is filled again: its windows' read vectors (one string and one vector of
    // base qualities per read) are overwritten in place instead of being freed by one thread and allocated anew by another.
    std::vector<WindowTask> tasks;
    std::vector<WindowJob> jobs;
    std::vector<size_t> jobOf;
    std::vector<PooledJob> pooled;       // --doPooled: per job, the window's active sets and what their EM slots returned (made by the compute stage)
    std::vector<int> toRelease;          // windows of the batch's previous use whose parsed haplotypes are no longer needed
    // several BAM pools: the windows in front of the batch (same chromosome, file order) whose read selection is replayed first
    struct Before { std::string tid; uint32_t leftPos, rightPos; int index; };
    std::vector<Before> lookBack;
};
typedef std::unique_ptr<Batch> BatchPtr;
typedef std::chrono::steady_clock::time_point TimePoint;

TimePoint now() { return std::chrono::steady_clock::now(); }
double seconds_since(const TimePoint &t0) { return std::chrono::duration<double>(now() - t0).count(); }

// ---------------------------------------------------------------- options, parsed once ----------------------------------------------------------------
struct Options {
    ObservationModelParameters obs; ReadSelectionParameters rsp; DiploidParameters dip;
    std::string varFile, hapFile, outputPrefix, libFile;
    std::string refFile;                 // --ref without --hapFile: the haplotypes are built in the run (empty: they come from hapFile)
    HaplotypeOptions hap;                // --ref mode: --maxHap, --skipMaxHap, --changeINStoN, --hostDistribution (maxHapReadProd is the run's)
    bool hostConvert;                    // --ref mode: convertHaplotypeAlignment on the host instead of the variants kernel
    std::string bamList;                 // --bamFiles LIST (read during set-up, behind the library file)
    std::vector<std::string> bamPaths;   // --bamFile, or LIST's files once set-up has read it
    double maxHapReadProd;
    int batchWindows, mergeBatches, cigarOpsCap, prepareThreads, computeThreads, packThreads, reduceThreads;
    long computeAhead;
    std::vector<int> devices;            // --devices 0,1,...: the engines are dealt out over these GPUs (batches are independent: no exchange between devices)
    bool faster, oneBased, prepareOnly, quiet, timing, longWindows, longWindowsFaster, wideDeletions, noLookBack, lateSkipsKnown, windowByWindow;
    bool realignedBAM, deviceCigars, deviceRealign, deviceRealignDiploid, checkDevicePair;
    bool deviceIndelKeys;                // --faster --deviceIndelKeys: the pairs' indel-map key counts come back instead of their alignments
    bool doPooled, doDiploid, hostEM;    // --doPooled: the pooled lines; the diploid lines too with --doDiploid, or when --doPooled is not given
    PooledParameters pool;               // --bayesa0, --bayesType
    bool keepAlignments;                 // the per-base alignments come back from the device (--faster without --deviceIndelKeys; --outputRealignedBAM without --deviceCigars)
    std::set<int> injectedLateSkips;
    int audit = 0, auditInject = -1;     // --audit N / --auditFaster N: windows audited per launch (0: off); --auditInject W (tests)
    bool auditFaster = false;            // the N came with --auditFaster: the --faster model against its shadow kernel
    unsigned long long auditSeed = 0;
    bool discover;                       // --discover: the discovery stage writes varFile (= disc.windowsFile()) before the loop starts
    DiscoverOptions disc;
    std::string vcfFile, vcfRef, sampleID;   // --vcf F: PREFIX.glf.txt -> F after the loop, with the FASTA of --ref
    std::string pooledVcfFile, pooledGlfFile;   // --pooledVcf F [--pooledGlf G]: PREFIX.glf.txt -> the pooled calls F (and their per-pool likelihoods G) after the loop
    PooledVcfOptions pooledVcf;              // ... with --numSamples, the FASTA of --ref and numBamFiles = the run's number of BAM files
};

const char *const kHelp =
    "dindel_gpu: the --analysis indels --doDiploid window loop with the likelihood step on the GPU\n"
    "  required: --bamFile F --varFile F --outputFile PREFIX and --ref FASTA or --hapFile F          (writes PREFIX.glf.txt)\n"
    "        or: --discover --bamFile F --ref FASTA --outputFile PREFIX        from a BAM and a FASTA alone: the candidates and the windows are made first\n"
    "  discover: --discover       the run starts with the discovery stage on the first device: candidate indels from the CIGARs of --bamFile, each\n"
    "                             realigned on the device, to PREFIX.variants.txt and PREFIX.libraries.txt (dindel_candidates --analysis getCIGARindels),\n"
    "                             then their windows to PREFIX.windows.txt (dindel_windows --oneFile), which the loop reads as its --varFile; the\n"
    "                             stage is a barrier in front of the loop; --hapFile cannot be given with it\n"
    "            [--tid NAME --region A-B]  candidates of that region only, from --bamFile or every file of --bamFiles (no PREFIX.libraries.txt)\n"
    "            [--minDist N]    candidates at most N bases apart share a window (default 20)\n"
    "            [--minCount N] [--maxCount M]  keep only candidates seen N ... M times (given one, the other is 2 / 10000000; default: keep all)\n"
    "            [--batchCandidates N] [--eventsCap N]  candidates per launch (65536) and indel events kept per alignment (8) of the realignment\n"
    "            [--useLibraries] PREFIX.libraries.txt becomes this run's --libFile (an explicit --libFile wins)\n"
    "            [--candidateVCF F[,G...]]  known sites: the indels of these VCFs (plain or .gz) become candidates beside the sample's own, through\n"
    "                             PREFIX.vcf.variants.txt (dindel_vcf2candidates), PREFIX.vcf.realigned.variants.txt (dindel_candidates --analysis\n"
    "                             realignCandidates, on the device) and PREFIX.candidates.txt, which the windows are made from; --minCount / --maxCount\n"
    "                             never filter them   [--minQual X] records with QUAL `.` or >= X (default 1)\n"
    "            [--vcfCandidatesOnly]  with --candidateVCF: no pass over the CIGARs of the BAM, the known sites alone\n"
    "  output:   [--vcf F]        after the loop, convert PREFIX.glf.txt to the VCF F (dindel_glf2vcf on that one file); needs --ref   [--sampleID ID]\n"
    "            [--pooledVcf F --numSamples N]  with --doPooled: after the loop, the pooled lines of PREFIX.glf.txt become the VCF F (dindel_pooled2vcf on that\n"
    "                             one file, --numBamFiles = the run's number of BAM files); needs --ref   [--pooledGlf G] and the called sites' likelihoods\n"
    "                             per pool go to G (dindel_pooled2glf)\n"
    "  haplotypes: --ref FASTA (with FASTA.fai)  every window's candidate haplotypes are built in the run from the reads it selected: the block\n"
    "                             tables and the alignment to the reference on the device, one launch each per batch of windows\n"
    "            [--maxHap N]     combinations the blocks are thinned to (default 8)      [--skipMaxHap N]  a window with more haplotypes is passed\n"
    "            [--changeINStoN] candidate insertions enter the haplotypes as N          over (default 200)\n"
    "            [--hostDistribution]  the block tables on the host instead of the device\n"
    "            [--hostConvert]  the variants of every alignment are made on the host from its slice instead of by the variants kernel\n"
    "            --hapFile F      the haplotypes come from a file instead (W / H / V / A records); with both, --hapFile wins and these have no effect\n"
    "  model:    [--faster] [--libFile F] [--filterHaplotypes] [--outputRealignedBAM] [--varFileIsOneBased]\n"
    "            [--doPooled]     the pooled analysis: one line per (candidate variant, pool) and window; alone it writes only those lines, with\n"
    "                             --doDiploid both (pooled first)   [--bayesa0 X] Dirichlet parameter (0.001)   [--bayesType all|singlevariant|priorpersite]\n"
    "            [--deviceCigars]  with --outputRealignedBAM: compute the realigned reads' CIGARs on the device and bring them back instead of the\n"
    "                             per-base alignments (same files); [--cigarOpsCap N] operations kept per read (default 8), reads with more\n"
    "                             are redone on the host, which recomputes their whole window with alignments once (one window at a time:\n"
    "                             a small N makes that the run's bottleneck); no effect without --outputRealignedBAM\n"
    "            [--deviceRealign]  with --doPooled --outputRealignedBAM: the device also picks each read's haplotype (pooled rule) and brings back that\n"
    "                             pair's CIGAR alone (same files; [--cigarOpsCap N] as above); refused with --doDiploid and with --faster; no effect\n"
    "                             without --outputRealignedBAM\n"
    "            [--deviceRealignDiploid]  with --doDiploid --outputRealignedBAM: the device picks and certifies every window's most likely haplotype\n"
    "                             pair, then each read's haplotype by the diploid rule, and brings back that pair's CIGAR alone (same files;\n"
    "                             [--cigarOpsCap N] as above); windows it cannot certify (ties, non-finite terms) are done on the host; refused with\n"
    "                             --faster, without --doDiploid and with --deviceRealign; no effect without --outputRealignedBAM; wins over\n"
    "                             --deviceCigars.  [--checkDevicePair] also choose every certified window's pair on the host and fail on a difference\n"
    "            [--longWindows]  compute windows with a haplotype > 766 bp or a read > 1024 bp (up to 4,094 / 4,096; with --maxLengthIndel >= 12\n"
    "                             also haplotypes > 574 bp) instead of skipping them; main model only: no effect with --faster\n"
    "            [--longWindowsFaster]  with --faster: compute windows with a haplotype > 766 bp or a read > 1024 bp (up to 4,094 / 4,096) instead of\n"
    "                             skipping them; no effect without --faster\n"
    "            [--wideDeletions]  accept --maxLengthIndel 32 and above (refused without it): implies --longWindows, every window then runs on the\n"
    "                             long-window kernel's wide build; with --faster it only lifts the parameter check; refused with --audit /\n"
    "                             --auditFaster at such a value\n"
    "            [--auditFaster N [--auditSeed S]]  --faster model: recompute N windows of every launch with the independent shadow kernel and\n"
    "                             compare them on the device with the --faster kernels' results (as --audit; needs --faster)\n"
    "            [--audit N [--auditSeed S]]  main model: recompute N windows of every launch with the long-window kernel and compare them on the\n"
    "                             device with the main kernels' results (same files; differences go to stderr, exit status 3; audit_windows=,\n"
    "                             audit_pairs=, audit_mismatches= in the timing line); refused with --faster\n"
    "            [--deviceIndelKeys]  with --faster: count every pair's indel-map keys on the device and bring 2 bytes per pair back instead of its\n"
    "                             per-base alignment (same PREFIX.glf.txt); no effect without --faster\n"
    "            [--maxRead N] [--maxReadLength N] [--minReadOverlap N] [--mapQualThreshold X] [--filterReadAux STR] [--pError X] [--pMut X] [--maxLengthIndel N]\n"
    "            [--flankRefSeq N] [--flankMaxMismatch N] [--priorSNP X] [--priorIndel X] [--capMapQualThreshold X] [--capMapQualFast X] [--maxHapReadProd N]\n"
    "  running:  [--batchWindows N] [--mergeBatches N] [--device D | --devices D0,D1,...] [--prepareThreads N] [--computeThreads N] [--packThreads N] [--reduceThreads N]\n"
    "            [--quiet] [--timing] [--prepareOnly]\n"
    "  files:    --varFile: the reference's window file; --hapFile: W / H / V / A records (host/window_io.hpp)\n";
// the options without a value; any other --NAME takes the next argument as its value, whatever its name
const char *const kFlags[] = {"varFileIsOneBased", "faster", "filterHaplotypes", "quiet", "doDiploid", "timing", "outputRealignedBAM", "prepareOnly", "noLookBack",
                              "lateSkipsKnown", "windowByWindow", "doPooled", "hostEM", "longWindows", "longWindowsFaster", "wideDeletions", "deviceCigars", "deviceRealign", "deviceRealignDiploid", "checkDevicePair", "deviceIndelKeys", "changeINStoN", "hostDistribution", "hostConvert", "discover", "useLibraries", "vcfCandidatesOnly"};

std::vector<int> commaInts(const std::string &list)      // "3,5,,8" -> 3 5 8
{
    std::vector<int> v;
    for (size_t i = 0; i <= list.size();) {
        size_t e = list.find(',', i);
        if (e == std::string::npos) e = list.size();
        if (e > i) v.push_back(atoi(list.substr(i, e - i).c_str()));
        i = e + 1;
    }
    return v;
}

// true: go on with `o`; false: leave with `exitCode` (0 help, 2 unknown argument or missing value, 1 missing required option)
bool parseOptions(int argc, char **argv, Options &o, int &exitCode)
{
    std::map<std::string, std::string> opt;
    for (int i = 1; i < argc; i++) if (!strcmp(argv[i], "--help") || !strcmp(argv[i], "-h")) { std::cout << kHelp; exitCode = 0; return false; }
    exitCode = 2;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a.compare(0, 2, "--") != 0) { std::cerr << "Unknown argument " << a << "\n"; return false; }
        a = a.substr(2);
        const size_t eq = a.find('=');
        if (eq != std::string::npos && eq > 0) { opt[a.substr(0, eq)] = a.substr(eq + 1); continue; }     // --NAME=VALUE
        bool flag = false;
        for (const char *f : kFlags) flag = flag || a == f;
        if (flag) opt[a] = "1";
        else if (i + 1 < argc) opt[a] = argv[++i];
        else { std::cerr << "Option --" << a << " needs a value\n"; return false; }
    }
    auto has = [&](const char *k) { return opt.find(k) != opt.end(); };
    auto num = [&](const char *k, double dflt) { return has(k) ? atof(opt[k].c_str()) : dflt; };
    exitCode = 1;
    if (has("deviceRealign") && has("doDiploid")) { std::cerr << "--deviceRealign cannot be given with --doDiploid: the realigned BAMs that stay are then the diploid step's, whose haplotype pair is computed on the host\n"; return false; }
    if (has("audit") && has("faster")) { std::cerr << "--audit cannot be given with --faster: that model's long-window kernel shares its main kernel's text, which is no independent check\n"; return false; }
    if (has("auditFaster") && !has("faster")) { std::cerr << "--auditFaster needs --faster: it audits that model's launches (--audit is the main model's)\n"; return false; }
    if ((has("auditInject") || has("auditSeed")) && !has("audit") && !has("auditFaster")) { std::cerr << "--auditInject and --auditSeed need --audit\n"; return false; }
    if (has("deviceRealign") && has("faster")) { std::cerr << "--deviceRealign cannot be given with --faster: realigned BAMs are written by the main model only\n"; return false; }
    if (has("deviceRealignDiploid") && has("faster")) { std::cerr << "--deviceRealignDiploid cannot be given with --faster: realigned BAMs are written by the main model only\n"; return false; }
    if (has("deviceRealignDiploid") && has("deviceRealign")) { std::cerr << "--deviceRealignDiploid cannot be given with --deviceRealign: one realigns by the diploid step's rule, the other by the pooled analysis'\n"; return false; }
    if (has("deviceRealignDiploid") && !has("doDiploid")) { std::cerr << "--deviceRealignDiploid needs --doDiploid: it realigns by the diploid step's rule\n"; return false; }
    o.discover = has("discover");
    for (const char *need : {"varFile", "outputFile"})
        if (!has(need) && !(o.discover && !strcmp(need, "varFile"))) { std::cerr << "Please specify --" << need << "\n"; return false; }
    if (o.discover && has("hapFile")) { std::cerr << "--discover builds the haplotypes in the run: --hapFile cannot be given with it\n"; return false; }
    if (o.discover && !has("ref")) { std::cerr << "Please specify --ref: --discover needs the reference FASTA\n"; return false; }
    if (has("vcf") && !has("ref")) { std::cerr << "Please specify --ref: --vcf needs the reference FASTA\n"; return false; }
    if (has("candidateVCF") && !o.discover) { std::cerr << "--candidateVCF adds known sites to the discovery stage: it needs --discover\n"; return false; }
    if (has("vcfCandidatesOnly") && !has("candidateVCF")) { std::cerr << "--vcfCandidatesOnly needs --candidateVCF\n"; return false; }
    if (has("vcfCandidatesOnly") && has("useLibraries")) { std::cerr << "--useLibraries needs the pass over the BAM file: with --vcfCandidatesOnly the discovery stage writes no library file\n"; return false; }
    if (has("vcfCandidatesOnly") && (has("minCount") || has("maxCount"))) {
        std::cerr << "--minCount / --maxCount filter the sample's own candidates: with --vcfCandidatesOnly there are none\n";
        return false;
    }
    if (!has("hapFile") && !has("ref")) { std::cerr << "Please specify --ref (haplotypes built in the run) or --hapFile (haplotypes from a file)\n"; return false; }
    if (!has("bamFile") && !has("bamFiles")) { std::cerr << "Error: Specify either --bamFile or --bamFiles." << std::endl; return false; }   // DInDel.cpp:4215-4218
    o.varFile = opt["varFile"]; o.outputPrefix = opt["outputFile"];
    if (has("vcf")) { o.vcfFile = opt["vcf"]; o.vcfRef = opt["ref"]; o.sampleID = has("sampleID") ? opt["sampleID"] : std::string("SAMPLE"); }
    if (o.discover) {                        // (the window file is ours: zero-based, whatever --varFileIsOneBased says)
        DiscoverOptions &d = o.disc;
        d.outputPrefix = o.outputPrefix; d.refFile = opt["ref"];
        o.varFile = d.windowsFile();
        if (has("region") != has("tid")) { std::cerr << "--tid and --region go together: --tid NAME --region A-B\n"; return false; }
        if (!has("region") && !has("bamFile") && !has("vcfCandidatesOnly")) { std::cerr << "Can extract the full set of indels from only BAM file at a time.\n"; return false; }
        if (has("region")) {
            d.haveRegion = true; d.tid = opt["tid"];
            try { parseRegion(opt["region"], d.start, d.end); } catch (const std::string &s) { std::cerr << s << "\n"; return false; }
        }
        if (has("candidateVCF")) {
            d.candidateVCF = opt["candidateVCF"]; d.vcfCandidatesOnly = has("vcfCandidatesOnly");
            if (d.candidateVCF.empty()) { std::cerr << "--candidateVCF needs the name of a VCF file\n"; return false; }
            try { if (has("minQual")) d.minQual = pythonFloat(opt["minQual"]); } catch (const std::string &e) { std::cerr << "--minQual: " << e << "\n"; return false; }
        }
        d.minDist = long(num("minDist", 20));
        d.filter = has("minCount") || has("maxCount");
        d.minCount = long(num("minCount", 2)); d.maxCount = long(num("maxCount", 10000000));
        d.candidates.batchCandidates = int(num("batchCandidates", d.candidates.batchCandidates));
        d.candidates.eventsCap = int(num("eventsCap", d.candidates.eventsCap));
        if (d.candidates.batchCandidates < 1) { std::cerr << "--batchCandidates must be at least 1\n"; exitCode = 2; return false; }
        if (d.candidates.eventsCap < 1 || d.candidates.eventsCap > DD_ALIGN_EVENTS_MAX_CAP) { std::cerr << "--eventsCap must be 1 ... 4096\n"; exitCode = 2; return false; }
        d.candidates.hostConvert = has("hostConvert"); d.candidates.quiet = has("quiet");
        if (has("useLibraries") && !has("libFile")) {
            if (d.haveRegion) { std::cerr << "--useLibraries needs a whole-file run: with --region the discovery stage writes no library file\n"; return false; }
            opt["libFile"] = d.librariesFile();
        }
    }
    if (has("hapFile")) o.hapFile = opt["hapFile"];                  // --hapFile wins when both are given
    else o.refFile = opt["ref"];
    if (has("bamFile")) o.bamPaths.push_back(opt["bamFile"]);        // --bamFile wins when both are given (DInDel.cpp:4220-4226)
    else o.bamList = opt["bamFiles"];
    o.faster = has("faster"); o.oneBased = has("varFileIsOneBased") && !o.discover; o.prepareOnly = has("prepareOnly"); o.quiet = has("quiet"); o.timing = has("timing");
    o.wideDeletions = has("wideDeletions");
    o.longWindows = has("longWindows") || o.wideDeletions; o.longWindowsFaster = has("longWindowsFaster");
    o.noLookBack = has("noLookBack"); o.lateSkipsKnown = has("lateSkipsKnown"); o.windowByWindow = has("windowByWindow");
    o.realignedBAM = has("outputRealignedBAM") && !o.faster;                      // `params.outputRealignedBAM && params.slower`, :589
    o.deviceCigars = o.realignedBAM && has("deviceCigars");                       // modifies --outputRealignedBAM only
    o.doPooled = has("doPooled"); o.doDiploid = has("doDiploid") || !o.doPooled; o.hostEM = has("hostEM");
    if (has("deviceRealign") && o.realignedBAM && !o.doPooled) { std::cerr << "--deviceRealign needs --doPooled: it realigns by the pooled analysis' rule\n"; return false; }
    o.deviceRealign = o.realignedBAM && has("deviceRealign");                     // modifies --doPooled --outputRealignedBAM only
    if (o.deviceRealign) o.deviceCigars = false;
    o.deviceRealignDiploid = o.realignedBAM && has("deviceRealignDiploid");       // modifies --doDiploid --outputRealignedBAM only
    o.checkDevicePair = o.deviceRealignDiploid && has("checkDevicePair");
    if (o.deviceRealignDiploid) o.deviceCigars = false;
    o.pool.a0 = num("bayesa0", o.pool.a0);
    if (has("bayesType")) o.pool.bayesType = opt["bayesType"];
    if (o.doPooled && !knownBayesType(o.pool.bayesType)) { std::cerr << "Unknown EM option" << std::endl; return false; }          // DInDel.cpp:2287-2288
    if (o.doPooled && !(o.pool.a0 > 0.0)) { std::cerr << "--bayesa0 must be positive\n"; exitCode = 2; return false; }
    // which of the reference's two realigned-BAM steps writes the files is easy to miss: said once, on stderr, like the reference's own notes
    if (o.doPooled && !o.doDiploid && o.realignedBAM && !o.quiet)
        std::cerr << "--doPooled --outputRealignedBAM without --doDiploid: the files are the pooled analysis' own (DInDel.cpp:498-520), every read on a haplotype "
                     "realigned to the first haplotype with the largest likelihood; with --doDiploid beside it they are the diploid step's\n";
    if (has("pooledVcf") && !o.doPooled) { std::cerr << "--pooledVcf converts the lines of the pooled analysis: it needs --doPooled\n"; return false; }
    if (has("pooledVcf") && !has("ref")) { std::cerr << "Please specify --ref: --pooledVcf needs the reference FASTA\n"; return false; }
    if (has("pooledVcf") && !has("numSamples")) { std::cerr << "Please specify --numSamples: --pooledVcf needs the number of samples in the pools\n"; return false; }
    if (has("pooledGlf") && !has("pooledVcf")) { std::cerr << "--pooledGlf writes the likelihoods of the sites --pooledVcf calls: it needs --pooledVcf\n"; return false; }
    if (has("pooledVcf")) {
        o.pooledVcfFile = opt["pooledVcf"]; o.pooledVcf.outputFile = o.pooledVcfFile; o.pooledVcf.refFile = opt["ref"];
        if (has("pooledGlf")) o.pooledGlfFile = opt["pooledGlf"];
        try { o.pooledVcf.numSamples = int(pytext::pyInt(opt["numSamples"])); } catch (const std::string &e) { std::cerr << "--numSamples: " << e << "\n"; return false; }
    }
    o.deviceIndelKeys = o.faster && has("deviceIndelKeys");                       // modifies --faster only
    o.keepAlignments = (o.faster && !o.deviceIndelKeys) || (o.realignedBAM && !o.deviceCigars && !o.deviceRealign && !o.deviceRealignDiploid);           // (the --faster model's indel count, DInDel.cpp:3529, needs hpos, or the device's count of its keys)
    o.cigarOpsCap = std::max(1, int(num("cigarOpsCap", 8)));
    ObservationModelParameters &obs = o.obs;
    obs.setCLIDefaultValues();
    obs.pError = num("pError", obs.pError); obs.pMut = num("pMut", obs.pMut);
    obs.maxLengthIndel = obs.maxLengthDel = int(num("maxLengthIndel", obs.maxLengthIndel));
    if (obs.maxLengthDel > DD_MAX_LENGTH_DEL && !o.wideDeletions) {
        std::cerr << "--maxLengthIndel " << obs.maxLengthDel << " needs --wideDeletions: the main kernels hold deletions up to " << DD_MAX_LENGTH_DEL << " bp\n";
        return false;
    }
    if (obs.maxLengthDel > DD_MAX_LENGTH_DEL && (has("audit") || has("auditFaster"))) {
        std::cerr << "--wideDeletions with --maxLengthIndel " << obs.maxLengthDel << " cannot be given with --audit / --auditFaster: the audit's shadow would be the same kernel\n";
        return false;
    }
    obs.padCover = int(num("flankRefSeq", obs.padCover)); obs.maxMismatch = int(num("flankMaxMismatch", obs.maxMismatch));
    obs.mapQualThreshold = num("capMapQualThreshold", obs.mapQualThreshold); obs.capMapQualFast = num("capMapQualFast", obs.capMapQualFast);
    ReadSelectionParameters &rsp = o.rsp;
    rsp.maxReads = size_t(num("maxRead", double(rsp.maxReads))); rsp.maxReadLength = size_t(num("maxReadLength", double(rsp.maxReadLength)));
    rsp.minReadOverlap = int(num("minReadOverlap", rsp.minReadOverlap)); rsp.mapQualThreshold = num("mapQualThreshold", rsp.mapQualThreshold);
    rsp.quiet = o.quiet; rsp.keepRecords = o.realignedBAM || !o.refFile.empty();   // (the haplotype stage reads CIGAR, flag and raw letters from the record)
    if (has("filterReadAux")) rsp.filterReadAux = opt["filterReadAux"];
    if (has("libFile")) {                    // the reference: --libFile switches mapUnmappedReads on (DInDel.cpp:4268-4272)
        o.libFile = opt["libFile"];
        rsp.mapUnmappedReads = obs.mapUnmappedReads = true;
    }
    o.dip.priorSNP = num("priorSNP", o.dip.priorSNP); o.dip.priorIndel = num("priorIndel", o.dip.priorIndel);
    o.dip.filterHaplotypes = has("filterHaplotypes"); o.dip.quiet = o.quiet;
    o.maxHapReadProd = num("maxHapReadProd", 10000000.0);
    if (!o.refFile.empty()) {                // DInDel.cpp:4127, :4132, :4139
        if (num("maxHap", 8) < 1 || num("skipMaxHap", 200) < 1) { std::cerr << "--maxHap and --skipMaxHap must be at least 1\n"; exitCode = 2; return false; }
        o.hap.maxHap = size_t(num("maxHap", 8)); o.hap.skipMaxHap = size_t(num("skipMaxHap", 200)); o.hap.maxHapReadProd = o.maxHapReadProd;
        o.hap.changeINStoN = has("changeINStoN"); o.hap.hostDistribution = has("hostDistribution");
    }
    o.hostConvert = has("hostConvert");
    {
    }
    o.batchWindows = std::max(1, int(num("batchWindows", 256)));
    o.devices = commaInts(has("devices") ? opt["devices"] : (has("device") ? opt["device"] : std::string("0")));
    if (o.devices.empty()) o.devices.push_back(0);
    o.disc.candidates.device = o.devices[0];
    // defaults measured on a 16-CPU share of an MI355X host (profiles/r03/n2_pipeline.md): per window the read selection costs
    // 0.10-0.20 ms of CPU, diploidGLF 0.09 ms, packing 0.025 ms; two engines per GPU keep it busy while one of them packs.  They
    // scale with the number of devices up to what the host has.
    unsigned hw = std::thread::hardware_concurrency();
    if (!hw) hw = 1;
    const unsigned nDev = unsigned(o.devices.size());
    o.computeThreads = std::max(1, int(num("computeThreads", (hw >= 8 ? 2.0 : 1.0) * double(nDev))));
    o.packThreads = int(num("packThreads", double(std::min(4u, std::max(1u, hw / (4 * nDev))))));   // host threads of each engine's packing (0: the engine's default)
    o.reduceThreads = std::max(1, int(num("reduceThreads", double(std::min(4u * nDev, std::max(1u, hw / 4))))));
    o.prepareThreads = std::max(1, int(num("prepareThreads", double(std::min(8u * nDev, std::max(1u, hw / 2))))));
    // prepared batches wait for the GPU in file order: room for one per prepare worker, so that a worker that was slow with the batch
    // at the head of the line (a descheduled thread on a busy host) does not idle the GPU while its successors are ready
    o.computeAhead = has("computeAhead") ? long(num("computeAhead", 0)) : long(std::max(o.computeThreads + 1, o.prepareThreads));
    // batches that are already waiting when an engine becomes free ride in one launch with the batch it takes (up to --mergeBatches of
    // them): the host stages keep their small batches, the GPU gets the larger launches it runs better (42.5 us per window in a launch of
    // 256 windows, 41.3 in one of 1,024, and one kernel boundary instead of four)
    // (default 4; 2 when the per-base alignments come back too: the page-locked result blocks of such a launch are 0.4 GB each, and
    // making them costs a 100,000-window run more than the launches save it; with --deviceCigars a realigned-BAM run brings none back: 4 again;
    // nor does --faster with --deviceIndelKeys)
    o.mergeBatches = std::max(1, int(num("mergeBatches", o.keepAlignments ? 2 : 4)));
    o.auditFaster = has("auditFaster");
    o.audit = std::max(0, int(num(o.auditFaster ? "auditFaster" : "audit", 0)));
    o.auditSeed = has("auditSeed") ? strtoull(opt["auditSeed"].c_str(), NULL, 10) : 0ull;
    o.auditInject = has("auditInject") ? int(num("auditInject", -1)) : -1;
    const std::vector<int> inject = commaInts(has("injectLateSkip") ? opt["injectLateSkip"] : std::string());
    o.injectedLateSkips.insert(inject.begin(), inject.end());
    return true;
}

// ---------------------------------------------------------------- the pipeline ----------------------------------------------------------------
// The main thread reads the window file (readWindowFile / flush); prepareWorker x --prepareThreads, computeWorker x --computeThreads and one
// writer (with --reduceThreads helpers per batch) run beside it.  Everything the stages share is a member; who writes it is said there.
class WindowLoop {
public:
    explicit WindowLoop(const Options &options);          // set-up: throws std::string
    int run();                                            // the exit code
    const std::vector<std::string> &bamPaths() const { return opt.bamPaths; }   // the run's BAM files (--bamFile, or the files of --bamFiles)
    long long auditMismatches() const { return n.auditMismatches.load(); }
private:
    void prepareWindow(ReadFetcher &fetcher, WindowTask &T);
    void fillPairPrior(WindowTask &T) const;
    void buildHaplotypes(const std::vector<WindowTask *> &tasks, IndexedFasta &fasta, int device);
    void prepareWorker(int pt);
    void computeWorker(int ct);
    void reduceWindow(WindowTask &T, const WindowJob *J, PooledJob *P = NULL);
    void pooledStage(std::vector<BatchPtr> &group, int device);
    void reduceBatch(Batch &B);
    void rePrepare(WindowTask &T);
    void writeBatch(Batch &B);
    void writer();
    bool flush();
    int readWindowFile();
    void report();

    void fail(const std::string &s);
    template <class F> void guarded(F stage);
    void configureStageEngine(LikelihoodEngine &engine) const;
    void noteAudit(const LikelihoodEngine &engine, const std::vector<const WindowTask *> &tasks);
    std::mutex audit_m;                  // the differences' lines on stderr, one report at a time
    WindowLikelihoods recomputeWithAlignments(const WindowTask &T);
    // the read buffer is reset behind this window: it was skipped, or (tests) its late skip was announced (DInDel.cpp:1401-1408)
    bool resetsBehind(bool skipped, int index) const { return skipped || (opt.lateSkipsKnown && opt.injectedLateSkips.count(index)); }

    // ---- fixed after set-up, read by every stage ----
    const TimePoint t_start;
    Options opt;
    LibraryCollection libraries;
    BamFileSet headerBam;                      // [0]: the first pool, opened before anything else happens ("Cannot open BAM file." / "Cannot open BAM index."); the header for --outputRealignedBAM
    std::unique_ptr<HaplotypeFixture> fixture; // (thread-safe: parsed on demand by the prepare workers, released through Batch::toRelease); none in --ref mode
    bool refMode;                              // --ref without --hapFile: buildHaplotypes makes each window's haplotypes
    const char *dumpReads;                     // DINDEL_DUMP_READS, diagnostics: what each window hands to the likelihood step
    bool pooled;                               // several BAM pools and no --noLookBack (diagnostics: every batch starts with an empty buffer)
    uint32_t bufferSpan;                       // a record fetched for a window has left the buffer this far on
    std::string glfFile;
    std::ofstream glfOutput;                   // written by the writer thread only
    OutputData glfData;                        // the output table: copied per window by reduceWindow
    double t_setup;

    // ---- the hand-overs: reader -> prepare -> compute -> reduce/write -> (recycled) -> reader ----
    BatchPool<Batch> recycled;
    Channel<BatchPtr> toPrepare;
    OrderedChannel<BatchPtr> toCompute, toReduce;
    std::atomic<int> computeLeft;              // the last compute worker to finish closes toReduce
    std::mutex done_m; std::condition_variable done_cv; bool reduceDone;     // the engines outlive the writer (see run())

    // ---- how the run ends badly: the first message wins ----
    std::mutex fatal_m; std::string fatal; std::atomic<int> fatalExit;

    // ---- --deviceCigars: the engine that recomputes a window WITH alignments for a read whose CIGAR did not fit; made at the first such read ----
    std::mutex fallback_m; std::unique_ptr<LikelihoodEngine> fallbackEngine;

    // ---- what the summary and --timing print.  Per-thread slots are written by their thread and summed after the joins. ----
    struct Counters {
        Counters(size_t np, size_t nc) : prepareOf(np, 0.0), computeOf(nc, 0.0), pooledOf(nc, 0.0), packOf(nc, 0.0), deviceOf(nc, 0.0), unpackOf(nc, 0.0), readyAt(nc, 0.0),
            reduce(0.0), reduceWork(0.0), launches(0), cigarFallbacks(0), hposBytes(0), cigarBytes(0), fallbackHposBytes(0), realignBytes(0), windows(0), skipped(0), rePrepared(0) {}
        std::vector<double> prepareOf, computeOf, pooledOf, packOf, deviceOf, unpackOf;
        std::vector<double> readyAt;           // when each engine had its device context, arena and streams
        double reduce;                         // the writer's busy time
        std::mutex reduceWork_m; double reduceWork;     // reduceWindow time summed over the writer and its helpers
        std::atomic<long> launches;            // engine calls with at least one job
        std::atomic<long> cigarFallbacks;      // reads redone with getCIGAR on the host (--deviceCigars)
        std::atomic<long long> hposBytes, cigarBytes, fallbackHposBytes;   // what the engines brought back from the device
        std::atomic<long long> realignBytes;   // ... of the realigned reads' arrays (--deviceRealign, --deviceRealignDiploid)
        std::atomic<long long> auditWindows{0}, auditPairs{0}, auditMismatches{0};   // --audit: summed over the launches
        std::atomic<long long> indelKeyBytes{0};   // ... of the indel-map key counts (--deviceIndelKeys)
        std::atomic<long> pairUncertified{0}, pairFallbackReads{0}, pairDisagreements{0};   // --deviceRealignDiploid, of the windows written: done on the host, reads redone there, --checkDevicePair
        long windows, skipped, rePrepared;     // the writer's
        std::vector<std::pair<double, long> > progress;   // the writer's: (seconds since start, windows written) after every batch
    } n;

    // ---- the reader's (main thread) ----
    struct Reader {
        Reader() : seq(0), nTasks(0) {}
        long seq; BatchPtr batch;
        size_t nTasks;                         // batch->tasks[nTasks...] are left-overs of an earlier use
        std::deque<Batch::Before> recent;      // the chromosome's windows so far that a later batch may need
    } reader;

    // ---- the writer's: several pools, the windows behind a late skip, re-prepared window by window from an empty buffer (see the header).  The
    //      fetcher, its BAM handles and the engine are made when the first late skip of the run is met. ----
    struct Redo {
        Redo() : active(false), first(false), reach(0) {}
        bool active, first;
        std::string tid; uint64_t reach;
        BamFileSet bams; std::unique_ptr<ReadFetcher> fetcher; std::unique_ptr<LikelihoodEngine> engine; std::unique_ptr<IndexedFasta> fasta;
    } redo;
};

WindowLoop::WindowLoop(const Options &options)
    : t_start(now()), opt(options), dumpReads(getenv("DINDEL_DUMP_READS")), glfFile(options.outputPrefix + ".glf.txt"), glfData(makeGLFOutputData(glfOutput)),
      toPrepare(size_t(options.prepareThreads) + 1), toCompute(std::max(1L, options.computeAhead)), toReduce(long(options.computeThreads) * options.mergeBatches + 1),
      computeLeft(options.computeThreads), reduceDone(false), fatalExit(1), n(size_t(options.prepareThreads), size_t(options.computeThreads))
{
    if (opt.rsp.mapUnmappedReads) libraries.addFromFile(opt.libFile);      // (only --libFile sets it)
    if (opt.bamPaths.empty()) {
        std::ifstream list(opt.bamList.c_str());             // one path per line, first word of the line (DInDel.cpp:64-88)
        if (!list.is_open()) { std::cout << "Cannot open file with BAM files:  " << opt.bamList << std::endl; throw std::string("File open error."); }
        std::string line;
        while (std::getline(list, line)) {
            std::istringstream is(line);
            std::string fname;
            is >> fname;
            if (!fname.empty()) opt.bamPaths.push_back(fname);
        }
        if (opt.bamPaths.empty()) throw std::string("No BAM file in ").append(opt.bamList);
    }
    headerBam.open(opt.bamPaths[0]);
    for (size_t i = 1; i < opt.bamPaths.size(); i++) { BamFileSet probe; probe.open(opt.bamPaths[i]); }     // every pool opens, or the run ends here
    refMode = !opt.refFile.empty();
    if (refMode) { IndexedFasta probe(opt.refFile); }        // the FASTA and its index open, or the run ends here; every worker opens its own
    else fixture.reset(new HaplotypeFixture(opt.hapFile));
    pooled = opt.bamPaths.size() > 1 && !opt.noLookBack;
    bufferSpan = 2u * uint32_t(libraries.getMaxInsertSize()) + 200u;
    glfOutput.open(glfFile.c_str());
    if (!glfOutput.is_open()) throw std::string("Cannot open file ").append(glfFile).append(" for writing.");
    glfData.outputLine(glfData.headerString());              // DInDel.cpp:1290-1291
    t_setup = seconds_since(t_start);
}

void WindowLoop::fail(const std::string &s)
{
    { std::lock_guard<std::mutex> lk(fatal_m); if (fatal.empty()) fatal = s; }
    toPrepare.abort(); toCompute.abort(); toReduce.abort();
}

// a stage's thread body: whatever it throws ends the run through fail()
template <class F> void WindowLoop::guarded(F stage)
{
    try { stage(); }
    catch (std::string &s) { fail(s); }
    catch (ReadFetcher::FatalError &e) { fatalExit = e.exitCode; fail(e.message); }   // the reference's exit() paths of getReads end the run here too
    catch (HaplotypeFixture::Error &e) { fail(e.message); }     // a malformed haplotype file ends the run, whichever window met it
    catch (std::exception &e) { fail(e.what()); }
}

// Engines, three configurations.  (a) the stage engine — compute workers and the writer's re-preparation: lazy views; per-base alignments only
// where a consumer reads them (Options::keepAlignments; diploidGLF reads scalars and covered flags only), device CIGARs and both long-window
// switches as asked.  (b) computeWorker adds its packing threads and the warm-up.  (c) recomputeWithAlignments' fallback engine.
void WindowLoop::configureStageEngine(LikelihoodEngine &engine) const
{
    engine.setThrowOnPositiveLikelihood(false);
    engine.setKeepAlignments(opt.keepAlignments);
    engine.setDeviceCigars(opt.deviceCigars, opt.cigarOpsCap);
    engine.setDeviceRealign(opt.deviceRealign, opt.cigarOpsCap);
    engine.setDeviceRealignDiploid(opt.deviceRealignDiploid, opt.cigarOpsCap);
    engine.setLongWindows(opt.longWindows);
    engine.setLongWindowsFaster(opt.longWindowsFaster);
    engine.setWideDeletions(opt.wideDeletions);
    if (opt.deviceIndelKeys) engine.setDeviceIndelKeys(true);
    if (opt.audit > 0 && opt.auditFaster) engine.setAuditFaster(opt.audit, opt.auditSeed);
    else if (opt.audit > 0) engine.setAudit(opt.audit, opt.auditSeed);
}

// --audit: the report of the engine's last call into the run's counters; every difference on stderr.  tasks[j]: the window of the call's job j.
void WindowLoop::noteAudit(const LikelihoodEngine &engine, const std::vector<const WindowTask *> &tasks)
{
    const LikelihoodEngine::AuditReport &A = engine.auditReport();
    n.auditWindows += A.windows; n.auditPairs += A.pairs; n.auditMismatches += A.mismatches;
    if (A.differences.empty()) return;
    std::lock_guard<std::mutex> lk(audit_m);
    for (const LikelihoodEngine::AuditDifference &d : A.differences) {
        const WindowTask *T = d.job >= 0 && size_t(d.job) < tasks.size() ? tasks[size_t(d.job)] : NULL;
        std::cerr << "audit mismatch: window " << (T ? T->index : -1) << " tid: " << (T ? T->tid : std::string("?")) << " pos: " << (T ? T->pos : 0u)
                  << " pair: " << d.pair << " field: " << LikelihoodEngine::auditFieldName(d.field) << "[" << d.index << "]"
                  << " main: 0x" << std::hex << d.primaryBits << (opt.auditFaster ? " shadow: 0x" : " long-window: 0x") << d.shadowBits << std::dec << std::endl;
    }
}

// (c) --deviceCigars: a read's CIGAR did not fit, its window is computed once more for the per-base alignments.  The engine must bring those
// back, so it keeps alignments (the default) and has no device CIGARs; realigned BAMs are main model only, so of the long-window switches
// setLongWindows alone matters.  One engine for the run, on devices[0], made at the first such read, used by one reduce helper at a time.
WindowLikelihoods WindowLoop::recomputeWithAlignments(const WindowTask &T)
{
    std::lock_guard<std::mutex> lk(fallback_m);
    if (!fallbackEngine) {
        fallbackEngine.reset(new LikelihoodEngine(opt.obs, opt.devices[0]));
        fallbackEngine->setThrowOnPositiveLikelihood(false);
        fallbackEngine->setLongWindows(opt.longWindows);
        fallbackEngine->setWideDeletions(opt.wideDeletions);
    }
    std::vector<WindowJob> one(1, T.job());
    fallbackEngine->computeLikelihoodsBatch(one);
    n.fallbackHposBytes += (long long)fallbackEngine->lastHposBytes;
    if (!one[0].error.empty()) throw std::string(one[0].error);
    return one[0].result;
}

// ---- --deviceRealignDiploid: the window's prior table, getHaplotypePrior per pair h1 <= h2 (it depends on the haplotypes and the candidates alone).
//      A prior that throws leaves NaN: the device then leaves the window to the host, whose maxLikelihoodPair throws the same string where it did. ----
void WindowLoop::fillPairPrior(WindowTask &T) const
{
    T.havePairPrior = false;
    if (!opt.deviceRealignDiploid || !T.computes() || !T.haps) return;
    const size_t H = T.haps->size();
    T.pairPrior.assign(H * H, 0.0);
    for (size_t h1 = 0; h1 < H; h1++)
        for (size_t h2 = h1; h2 < H; h2++) {
            try { T.pairPrior[h1 * H + h2] = getHaplotypePrior((*T.haps)[h1], (*T.haps)[h2], int(T.leftPos), T.candidates, opt.dip); }
            catch (std::string &) { T.pairPrior[h1 * H + h2] = std::numeric_limits<double>::quiet_NaN(); }
        }
    T.havePairPrior = true;
}

// ---- one window's read selection and haplotypes (the prepare workers; the writer's re-preparation behind a late skip) ----
void WindowLoop::prepareWindow(ReadFetcher &fetcher, WindowTask &T)
{
    try {
        fetcher.getReads(T.tid, T.fileLeftPos, T.fileRightPos, T.reads);
        if (!refMode) {                                                         // --ref: buildHaplotypes follows, for the whole batch
            const WindowHaplotypes *wh = fixture->find(T.index);
            if (!wh) throw std::string("no haplotypes for this window in the haplotype file");
            T.haps = &wh->haps; T.leftPos = wh->leftPos; T.rightPos = wh->rightPos;
            if (double(T.reads.size() * T.haps->size()) > opt.maxHapReadProd) {     // :395-399
                std::stringstream os;
                os << "skipped_numhap_times_numread>" << long(opt.maxHapReadProd);
                throw os.str();
            }
        }
    } catch (std::string &s) {
        T.message = skippedMessage(s);
        T.skipped = true;
    }
    if (dumpReads) {
        std::ofstream df((std::string(dumpReads) + "." + std::to_string(T.index)).c_str());
        df.precision(17);
        for (size_t r = 0; r < T.reads.size(); r++) {
            const Read &R = T.reads[r];
            df << R.qname << " " << R.poolID << " " << int32_t(R.pos) << " " << R.mapQual << " " << R.matePos << " " << R.mateLen << " " << R.isUnmapped() << " " << R.isPaired()
               << " " << R.mateIsUnmapped() << " " << R.mateIsReverse() << " " << R.mateSameTid << " " << R.posStat.first << " "
               << (R.library ? R.library->getMaxInsertSize() : -1) << " " << R.seq.seq << "\n";
        }
    }
}

// ---- --ref: getHaplotypes (DInDel.cpp:1526-1645) for the windows of a batch whose reads are selected, and what empiricalDistributionMethod
//      does with its result in front of the likelihood step (:393-405).  One block-table launch and one alignment launch for all of them
//      (getHaplotypesBatch, alignHaplotypesBatch); the variants of each alignment come from the variants kernel behind the alignment
//      launch, or with --hostConvert from convertHaplotypeAlignment on the host.
//      What the reference THROWS here becomes the window's skipped line, and a late skip: read selection is over, the reference empties
//      its read buffer behind the window (:1401-1408).  Where getHaplotypes RETURNS true the window is passed over: a cerr line, no row.
//      A library error (no device, out of memory) is thrown on and ends the run. ----
void WindowLoop::buildHaplotypes(const std::vector<WindowTask *> &tasks, IndexedFasta &fasta, int device)
{
    auto thrown = [](WindowTask &T, const std::string &what) { T.message = skippedMessage(what); T.skipped = true; T.lateSkip = true; T.haps = NULL; };
    auto upper = [](std::string s) { for (size_t i = 0; i < s.size(); i++) s[i] = char(toupper((unsigned char)s[i])); return s; };
    HapBatchData data;
    std::vector<WindowCandidates> wins;
    std::vector<WindowTask *> of;                           // wins[k] belongs to *of[k]
    for (size_t i = 0; i < tasks.size(); i++) {
        WindowTask &T = *tasks[i];
        if (T.skipped) continue;
        // :1530-1532, and getRefSeq (:269-287), which throws when nothing of the piece lies on the sequence
        const uint32_t rs = int(T.fileLeftPos) > opt.rsp.minReadOverlap ? T.fileLeftPos - uint32_t(opt.rsp.minReadOverlap) : 0u;
        const uint32_t re = T.fileRightPos + uint32_t(opt.rsp.minReadOverlap);
        std::string piece;
        try { piece = refPiece(fasta, T.tid, long(rs) + 1, long(re) + 1); } catch (std::string &e) { thrown(T, e); continue; }
        if (piece.empty()) { thrown(T, "faidx error: len==0"); continue; }
        data.addWindow(int32_t(rs), piece);
        addWindowReads(data, T.reads);
        WindowCandidates w;
        w.leftPos = T.fileLeftPos; w.rightPos = T.fileRightPos; w.variants = T.candidates.variants; w.nReads = T.reads.size();
        wins.push_back(w);
        of.push_back(&T);
    }
    if (wins.empty()) return;
    HaplotypeOptions hopt = opt.hap;
    hopt.device = device;
    getHaplotypesBatch(data, wins, hopt);
    std::vector<WindowHaplotypes> toAlign;
    std::vector<std::string> refSeqs;
    std::vector<WindowTask *> aligned;
    auto tooMany = [&](WindowTask &T, size_t nHaps) {       // :395-399
        if (!(double(T.reads.size() * nHaps) > opt.maxHapReadProd)) return false;
        std::stringstream os;
        os << "skipped_numhap_times_numread>" << long(opt.maxHapReadProd);
        thrown(T, os.str());
        return true;
    };
    for (size_t k = 0; k < wins.size(); k++) {
        WindowTask &T = *of[k];
        const WindowCandidates &w = wins[k];
        std::ostringstream note;
        if (w.returnedSkip) {                               // :1569 (no haplotypes yet) / :1581 (all of them, unaligned): :395 still runs
            note << "tid: " << T.tid << " pos: " << T.pos << " " << w.message << "\n";
            if (!tooMany(T, w.hapsAtSkip)) { T.passedOver = true; note << "tid: " << T.tid << " pos:  " << T.pos << " SKIPPING!\n"; }
        } else if (w.message == "Blocks are not consecutive.") {     // :1636-1639
            note << "tid: " << T.tid << "pos: " << T.pos << w.message << "\n";
            thrown(T, "hapblock");
        } else if (!w.message.empty()) thrown(T, w.message);
        else {
            WindowHaplotypes in;
            in.index = T.index; in.leftPos = w.leftPos; in.rightPos = w.rightPos;
            for (size_t h = 0; h < w.haps.size(); h++) in.haps.push_back(Haplotype(w.haps[h]));
            std::string ref;                                // :1461: getRefSeq(leftPos + 1, rightPos + 1) of the selected blocks
            try { ref = upper(refPiece(fasta, T.tid, long(w.leftPos) + 1, long(w.rightPos) + 1)); } catch (std::string &e) { thrown(T, e); }
            if (!T.skipped && ref.empty()) thrown(T, "faidx error: len==0");
            if (!T.skipped) { toAlign.push_back(in); refSeqs.push_back(ref); aligned.push_back(&T); }
        }
        T.note = note.str();
    }
    std::vector<std::string> errors;
    // Haplotype::refHpos is read by the realigned BAMs' CIGARs only (realignedCigars, the device CIGARs' hap_ref_pos)
    alignHaplotypesBatch(toAlign, refSeqs, device, &errors, opt.hostConvert ? CONVERT_HOST : CONVERT_DEVICE, opt.realignedBAM);
    for (size_t k = 0; k < toAlign.size(); k++) {
        WindowTask &T = *aligned[k];
        if (!errors[k].empty()) { thrown(T, errors[k]); continue; }
        if (tooMany(T, toAlign[k].haps.size())) continue;   // on what the overhang filter and the duplicate-reference removal left
        T.built.swap(toAlign[k].haps);
        T.haps = &T.built; T.leftPos = toAlign[k].leftPos; T.rightPos = toAlign[k].rightPos;
    }
}

// ---- prepare: whole batches side by side (own BAM handles and read buffer per worker), handed on in file order ----
void WindowLoop::prepareWorker(int pt)
{
    guarded([&] {
        BamFileSet bams(opt.bamPaths);
        ReadFetcher fetcher(bams.pointers(), libraries, opt.rsp);
        std::vector<Read> replayed;
        std::unique_ptr<IndexedFasta> fasta;
        if (refMode && !opt.prepareOnly) fasta.reset(new IndexedFasta(opt.refFile));    // --prepareOnly stops in front of the haplotype stage
        std::vector<WindowTask *> all;
        BatchPtr b;
        while (toPrepare.pop(b)) {
            const TimePoint t0 = now();
            if (fixture) for (size_t i = 0; i < b->toRelease.size(); i++) fixture->release(b->toRelease[i]);      // noted by the writer at the batch's previous use
            b->toRelease.clear();
            std::string oldTid;
            bool primed = false;
            if (!b->lookBack.empty()) {               // several pools: bring the buffer to the state the windows in front left it in
                fetcher.newChromosome();
                for (size_t k = 0; k < b->lookBack.size(); k++) {
                    const Batch::Before &W = b->lookBack[k];
                    bool skipped = false;
                    try { fetcher.getReads(W.tid, W.leftPos, W.rightPos, replayed); } catch (std::string &) { skipped = true; }
                    fetcher.windowDone(resetsBehind(skipped, W.index), W.leftPos);
                }
                oldTid = b->lookBack.back().tid;
                primed = true;
            }
            for (size_t i = 0; i < b->tasks.size(); i++) {
                WindowTask &T = b->tasks[i];
                if ((i == 0 && !primed) || T.tid != oldTid) { fetcher.newChromosome(); oldTid = T.tid; }     // DInDel.cpp:1327-1333
                prepareWindow(fetcher, T);
                fetcher.windowDone(resetsBehind(T.skipped, T.index), T.fileLeftPos);                         // :1401-1408
            }
            if (fasta) {
                all.clear();
                for (size_t i = 0; i < b->tasks.size(); i++) all.push_back(&b->tasks[i]);
                buildHaplotypes(all, *fasta, opt.devices[size_t(pt) % opt.devices.size()]);
            }
            for (size_t i = 0; i < b->tasks.size(); i++) fillPairPrior(b->tasks[i]);
            n.prepareOf[size_t(pt)] += seconds_since(t0);
            const long seq = b->seq;
            if (!toCompute.push(seq, b)) break;
        }
    });
}

// ---- compute: every prepared window of a batch in one call; --computeThreads engines take batches in turn, so that one
//      packs its batch (host) while the other's is on the GPU ----
void WindowLoop::computeWorker(int ct)
{
    guarded([&] {
        BatchPtr b;
        LikelihoodEngine engine(opt.obs, opt.devices[size_t(ct) % opt.devices.size()]);
        configureStageEngine(engine);
        if (opt.packThreads > 0) engine.setHostThreads(opt.packThreads);
        if (!opt.prepareOnly) engine.warmUp(size_t(opt.batchWindows) * size_t(opt.mergeBatches) * 8 * 200);     // while the first batches are being prepared
        n.readyAt[size_t(ct)] = seconds_since(t_start);
        std::vector<BatchPtr> group;
        std::vector<WindowJob> merged;
        bool open = true;
        while (open && toCompute.pop(b)) {
            const TimePoint t0 = now();
            group.clear();
            group.push_back(std::move(b));
            while (int(group.size()) < opt.mergeBatches && toCompute.tryPop(b)) group.push_back(std::move(b));
            size_t nJobs = 0;
            for (size_t g = 0; g < group.size(); g++) {
                Batch &B = *group[g];
                B.jobOf.assign(B.tasks.size(), size_t(-1));
                for (size_t i = 0; i < B.tasks.size(); i++) if (B.tasks[i].computes()) { B.jobOf[i] = B.jobs.size(); B.jobs.push_back(B.tasks[i].job()); }
                nJobs += B.jobs.size();
            }
            if (nJobs > 0 && !opt.prepareOnly) {
                // one call for the group: the jobs travel through one vector and go back to their batches, in the same order, with their views
                std::vector<WindowJob> *jobs = &group[0]->jobs;
                if (group.size() > 1) {
                    merged.clear();
                    for (size_t g = 0; g < group.size(); g++)
                        for (size_t j = 0; j < group[g]->jobs.size(); j++) merged.push_back(std::move(group[g]->jobs[j]));
                    jobs = &merged;
                }
                if (opt.audit > 0) {                     // --auditInject: the job of that window, if this launch holds it
                    size_t at = 0;
                    for (size_t g = 0; g < group.size(); g++)
                        for (size_t i = 0; i < group[g]->tasks.size(); i++)
                            if (group[g]->jobOf[i] != size_t(-1)) { if (group[g]->tasks[i].index == opt.auditInject) engine.setAuditInject(int(at)); at++; }
                }
                if (opt.faster) engine.computeLikelihoodsFasterBatch(*jobs); else engine.computeLikelihoodsBatch(*jobs);
                if (opt.audit > 0) {
                    std::vector<const WindowTask *> taskOf;
                    for (size_t g = 0; g < group.size(); g++)
                        for (size_t i = 0; i < group[g]->tasks.size(); i++) if (group[g]->jobOf[i] != size_t(-1)) taskOf.push_back(&group[g]->tasks[i]);
                    noteAudit(engine, taskOf);
                }
                if (group.size() > 1) {
                    size_t at = 0;
                    for (size_t g = 0; g < group.size(); g++)
                        for (size_t j = 0; j < group[g]->jobs.size(); j++) group[g]->jobs[j] = std::move(merged[at++]);
                    merged.clear();
                }
                if (opt.doPooled) {
                    const TimePoint p0 = now();
                    pooledStage(group, opt.devices[size_t(ct) % opt.devices.size()]);
                    n.pooledOf[size_t(ct)] += seconds_since(p0);
                }
                n.packOf[size_t(ct)] += engine.lastPackSeconds; n.deviceOf[size_t(ct)] += engine.lastDeviceSeconds; n.unpackOf[size_t(ct)] += engine.lastUnpackSeconds;
                n.hposBytes += (long long)engine.lastHposBytes; n.cigarBytes += (long long)engine.lastCigarBytes; n.realignBytes += (long long)engine.lastRealignBytes;
                n.indelKeyBytes += (long long)engine.lastIndelKeyBytes;
                n.launches++;
            }
            n.computeOf[size_t(ct)] += seconds_since(t0);
            for (size_t g = 0; g < group.size() && open; g++) { const long seq = group[g]->seq; if (!toReduce.push(seq, group[g])) open = false; }
        }
        group.clear();
        b.reset();
        if (--computeLeft == 0) toReduce.close();
        // the batches still being reduced hold views into this engine's result blocks: wait for the writer
        std::unique_lock<std::mutex> lk(done_m);
        done_cv.wait(lk, [&] { return reduceDone; });
    });
}

// ---- --doPooled, compute stage: the active sets and masks of every computed window of the group, then all their EM slots in one launch
//      (--hostEM: on the CPU).  The ll go up again from the result block: the engine's own copy on the device belongs to its call. ----
void WindowLoop::pooledStage(std::vector<BatchPtr> &group, int device)
{
    std::vector<PooledPlan *> plans;
    std::vector<const PooledWindow *> wins;
    for (size_t g = 0; g < group.size(); g++) {
        Batch &B = *group[g];
        B.pooled.assign(B.jobs.size(), PooledJob());
        for (size_t i = 0; i < B.tasks.size(); i++) {
            if (B.jobOf[i] == size_t(-1)) continue;
            const WindowJob &J = B.jobs[B.jobOf[i]];
            const WindowTask &T = B.tasks[i];
            if (!J.error.empty() || !J.result.valid() || opt.injectedLateSkips.count(T.index)) continue;
            PooledJob &P = B.pooled[B.jobOf[i]];
            pooledWindowOf(*T.haps, T.reads, J.result, opt.dip, P.win);
            pooledPlan(*T.haps, P.win, T.leftPos, T.candidates, opt.dip, opt.pool.bayesType, P.plan);
            plans.push_back(&P.plan);
            wins.push_back(&P.win);
        }
    }
    if (!plans.empty()) pooledRunEM(plans, wins, opt.pool, opt.hostEM, device, std::max(1, opt.packThreads));
}

// ---- one window's lines: diploidGLF (+ the realigned BAM), or the skipped-window line (the reduce helpers; the writer's
//      re-preparation behind a late skip) ----
void WindowLoop::reduceWindow(WindowTask &T, const WindowJob *J, PooledJob *P)
{
    std::ostringstream os;
    OutputData local = glfData;
    local.out = &os;
    T.pairUncertified = T.pairFallbackReads = T.pairDisagreements = 0;
    if (T.computes()) {
        try {
            if (opt.injectedLateSkips.count(T.index)) throw std::string("hapSize error.");       // tests (--injectLateSkip)
            if (J) {
                if (!J->error.empty()) throw std::string(J->error);
                // like the reference, diploidGLF writes its lines as it goes: if it throws half-way ("genotyping
                // error"), the lines already written stay and the skipped-window line follows them
                if (opt.doPooled) {                                          // DInDel.cpp:411-470: in front of the diploid analysis
                    PooledJob own;
                    if (!P || !P->plan.ready) {                              // a window the writer re-did: its one launch here
                        pooledWindowOf(*T.haps, T.reads, J->result, opt.dip, own.win);
                        pooledPlan(*T.haps, own.win, T.leftPos, T.candidates, opt.dip, opt.pool.bayesType, own.plan);
                        pooledRunEM(std::vector<PooledPlan *>(1, &own.plan), std::vector<const PooledWindow *>(1, &own.win), opt.pool, opt.hostEM, opt.devices[0], 1);
                        P = &own;
                    }
                    pooledLines(*T.haps, T.reads, P->win, P->plan, T.pos, T.leftPos, T.rightPos, local, T.index, T.tid, T.candidates, opt.dip, opt.pool.bayesType,
                                opt.bamPaths.size());
                }
                if (opt.doPooled && !opt.doDiploid && opt.realignedBAM) {    // DInDel.cpp:498-520: the pooled analysis' own file (with --doDiploid its step below overwrites it)
                    std::vector<CIGAR> cigars;
                    long fallbacks = 0;
                    pooledRealignedCigars(*T.haps, T.reads, J->result, int(T.leftPos), cigars, [&]() { return recomputeWithAlignments(T); }, &fallbacks);
                    n.cigarFallbacks += fallbacks;
                    std::vector<int> onHap(T.reads.size());
                    for (size_t r = 0; r < onHap.size(); r++) onHap[r] = J->result.onHap(r);
                    writeRealignedBAMFile(realignedBAMFileName(opt.outputPrefix, T.index, T.tid, T.leftPos, T.rightPos, opt.rsp.minReadOverlap),
                                          cigars, T.reads, onHap, headerBam[0]);
                }
                if (opt.doDiploid) diploidGLF(*T.haps, T.reads, J->result, T.pos, T.leftPos, T.rightPos, local, T.index, T.tid, T.candidates, opt.dip, "dip");
                if (opt.realignedBAM && opt.doDiploid) {                     // DInDel.cpp:589-620
                    std::vector<CIGAR> cigars;
                    long fallbacks = 0;
                    if (J->result.hasDevicePair()) {                         // --deviceRealignDiploid: a certified window's pair and rows are the device's
                        long uncertified = 0;
                        const std::pair<int, int> used = diploidDeviceRealignedCigars(*T.haps, T.reads, J->result, int(T.leftPos), T.candidates, opt.dip, int(T.leftPos),
                                                                                     cigars, [&]() { return recomputeWithAlignments(T); }, &fallbacks, &uncertified);
                        T.pairUncertified = uncertified; T.pairFallbackReads = fallbacks;
                        if (opt.checkDevicePair && !uncertified &&
                            maxLikelihoodPair(*T.haps, T.reads, J->result, int(T.leftPos), T.candidates, opt.dip) != used) T.pairDisagreements = 1;
                    } else {
                        const std::pair<int, int> best = maxLikelihoodPair(*T.haps, T.reads, J->result, int(T.leftPos), T.candidates, opt.dip);
                        realignedCigars(*T.haps, T.reads, J->result, best, int(T.leftPos), cigars, [&]() { return recomputeWithAlignments(T); }, &fallbacks);
                    }
                    n.cigarFallbacks += fallbacks;
                    std::vector<int> onHap(T.reads.size());
                    for (size_t r = 0; r < onHap.size(); r++) onHap[r] = J->result.onHap(r);
                    writeRealignedBAMFile(realignedBAMFileName(opt.outputPrefix, T.index, T.tid, T.leftPos, T.rightPos, opt.rsp.minReadOverlap),
                                          cigars, T.reads, onHap, headerBam[0]);
                }
            }
        } catch (std::string &s) {
            T.message = skippedMessage(s);
            T.skipped = true;
            T.lateSkip = true;                                           // after read selection: the reference resets its read buffer behind it (:1404-1405)
        }
    }
    if (T.skipped) local.output(skippedWindowLine(local, T.message, T.index, T.tid, T.fileLeftPos, T.fileRightPos));
    T.lines = os.str();
}

// ---- reduce: windows of a batch side by side (the writer and --reduceThreads - 1 helpers), each into its own buffer ----
void WindowLoop::reduceBatch(Batch &B)
{
    std::atomic<size_t> next(0);
    // a helper thread must not let anything escape (std::terminate): whatever diploidGLF, the CIGAR step or the BAM writer
    // throws beside the reference's strings ends the run through fail(), and the helpers stop taking windows
    auto work = [&]() {
        const TimePoint w0 = now();
        try {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= B.tasks.size()) break;
                const bool computed = B.tasks[i].computes() && !opt.prepareOnly;
                reduceWindow(B.tasks[i], computed ? &B.jobs[B.jobOf[i]] : NULL, computed && B.jobOf[i] < B.pooled.size() ? &B.pooled[B.jobOf[i]] : NULL);
            }
        } catch (std::exception &e) { next.store(B.tasks.size()); fail(std::string("reduce: ") + e.what()); }
        catch (...) { next.store(B.tasks.size()); fail("reduce: unknown exception"); }
        const double dt = seconds_since(w0);
        std::lock_guard<std::mutex> lk(n.reduceWork_m);
        n.reduceWork += dt;
    };
    std::vector<std::thread> pool;
    const int nt = int(std::min<size_t>(size_t(opt.reduceThreads), B.tasks.size()));
    for (int t = 1; t < nt; t++) pool.push_back(std::thread(work));
    work();
    for (size_t t = 0; t < pool.size(); t++) pool[t].join();
}

// the writer's re-preparation of one window (behind a late skip; every window under --windowByWindow): read selection from redo's own
// buffer, likelihoods on redo's own stage engine, the same reduce step; T's lines replace what the pipeline prepared ahead
void WindowLoop::rePrepare(WindowTask &T)
{
    if (!redo.fetcher) {
        redo.bams = BamFileSet(opt.bamPaths);
        redo.fetcher.reset(new ReadFetcher(redo.bams.pointers(), libraries, opt.rsp));
    }
    if (redo.first) { redo.fetcher->newChromosome(); redo.reach = uint64_t(T.fileRightPos) + bufferSpan; redo.first = false; }   // the reset of DInDel.cpp:1404-1405
    T.skipped = false; T.lateSkip = false; T.passedOver = false; T.message = "ok"; T.note.clear(); T.haps = NULL; T.havePairPrior = false;
    prepareWindow(*redo.fetcher, T);
    if (refMode && !opt.prepareOnly) {
        if (!redo.fasta) redo.fasta.reset(new IndexedFasta(opt.refFile));
        buildHaplotypes(std::vector<WindowTask *>(1, &T), *redo.fasta, opt.devices[0]);
    }
    fillPairPrior(T);
    std::vector<WindowJob> one;
    if (T.computes() && !opt.prepareOnly) {
        if (!redo.engine) {
            redo.engine.reset(new LikelihoodEngine(opt.obs, opt.devices[0]));
            configureStageEngine(*redo.engine);
        }
        one.push_back(T.job());
        if (opt.audit > 0 && T.index == opt.auditInject) redo.engine->setAuditInject(0);
        if (opt.faster) redo.engine->computeLikelihoodsFasterBatch(one); else redo.engine->computeLikelihoodsBatch(one);
        if (opt.audit > 0) noteAudit(*redo.engine, std::vector<const WindowTask *>(1, &T));
        n.hposBytes += (long long)redo.engine->lastHposBytes; n.cigarBytes += (long long)redo.engine->lastCigarBytes; n.realignBytes += (long long)redo.engine->lastRealignBytes;
        n.indelKeyBytes += (long long)redo.engine->lastIndelKeyBytes;
    }
    reduceWindow(T, one.empty() ? NULL : &one[0]);
    redo.fetcher->windowDone(T.skipped, T.fileLeftPos);
    n.rePrepared++;
}

// ---- write: a reduced batch's windows in window order; a late skip with several pools starts the redo chain ----
void WindowLoop::writeBatch(Batch &B)
{
    for (size_t i = 0; i < B.tasks.size(); i++) {
        WindowTask &T = B.tasks[i];
        if (opt.windowByWindow) {
            // (tests, diagnostics) EVERY window is re-done — read selection from the writer's own buffer, likelihoods, genotyping — one after the
            // other, i.e. the reference's loop as it stands (DInDel.cpp:1310-1411); what the pipeline prepared ahead is ignored
            if (T.tid != redo.tid || !redo.fetcher) { redo.first = true; redo.tid = T.tid; }     // DInDel.cpp:1327-1333
            rePrepare(T);
        } else if (redo.active) {
            // (a new chromosome resets the buffer in both histories; beyond `reach` no record of the reset's moment is left)
            if ((redo.first && T.tid != redo.tid) || (!redo.first && (T.tid != redo.tid || uint64_t(T.fileLeftPos) >= redo.reach))) redo.active = false;
            else rePrepare(T);
        }
        if (T.lateSkip && pooled && !opt.lateSkipsKnown && !opt.windowByWindow) { redo.active = true; redo.first = true; redo.tid = T.tid; }
        if (!T.note.empty()) std::cerr << T.note << std::flush;                                            // DInDel.cpp:1570, :1582, :1637, :404
        if (T.skipped) {
            std::cerr << "skipped " << T.tid << " " << T.pos << " reason: " << T.message << std::endl;     // DInDel.cpp:1383
            n.skipped++;
        }
        glfOutput << T.lines;
        n.pairUncertified += T.pairUncertified; n.pairFallbackReads += T.pairFallbackReads; n.pairDisagreements += T.pairDisagreements;   // of the lines written: a window re-done counts once
        n.windows++;
    }
    glfOutput.flush();
    n.progress.push_back(std::make_pair(seconds_since(t_start), n.windows));
}

void WindowLoop::writer()
{
    guarded([&] {                                         // (the re-preparation behind a late skip reads the BAM files too)
        BatchPtr b;
        while (toReduce.pop(b)) {
            const TimePoint t0 = now();
            reduceBatch(*b);
            writeBatch(*b);
            // the haplotypes of these windows can go: noted here, dropped by the prepare worker that takes the batch next
            // (side by side with the others, not in this thread's serial part)
            for (size_t i = 0; i < b->tasks.size(); i++) if (b->tasks[i].haps) { if (fixture) b->toRelease.push_back(b->tasks[i].index); b->tasks[i].haps = NULL; }
            b->jobs.clear();                                              // drops the batch's views: its result block can be reused
            b->jobOf.clear();
            b->pooled.clear();
            recycled.give(b);
            n.reduce += seconds_since(t0);
        }
    });
    redo.engine.reset(); redo.fetcher.reset(); redo.fasta.reset();            // made by this thread, dropped by it
}

// ---- the window file, in file order (main thread) ----
bool WindowLoop::flush()                                  // the reader's batch goes to the prepare workers; false: they are gone
{
    Batch &B = *reader.batch;
    B.seq = reader.seq++;
    B.tasks.resize(reader.nTasks);
    B.lookBack.clear();
    if (pooled && reader.nTasks) {
        // windows of recent[] in front of the batch's first one; the replay starts at the last of them whose own fetch
        // (everything up to rightPos + maxInsert) has left the buffer when the batch's first window is selected
        std::deque<Batch::Before> &recent = reader.recent;
        const WindowTask &first = B.tasks[0];
        auto gone = [&](const Batch::Before &W) {          // W's own fetch has left the buffer by the batch's first window (or never was in it)
            return W.tid != first.tid || uint64_t(W.rightPos) + bufferSpan <= uint64_t(first.fileLeftPos);
        };
        const size_t n0 = recent.size() - reader.nTasks;                           // recent[] ends with this batch's windows
        size_t from = n0;
        while (from > 0 && recent[from - 1].tid == first.tid) { from--; if (gone(recent[from])) break; }
        B.lookBack.assign(recent.begin() + long(from), recent.begin() + long(n0));
        while (recent.size() > reader.nTasks + 1 && gone(recent[1])) recent.pop_front();   // recent[0] stays a start later batches can use
    }
    const bool ok = toPrepare.push(reader.batch);
    reader.batch = recycled.take();
    reader.nTasks = 0;
    return ok;
}

int WindowLoop::readWindowFile()                          // 1: the file is not sorted (what was read so far is still written)
{
    int rc = 0;
    VariantFile vf(opt.varFile);
    int index = 0;
    std::string oldTid("-1");
    uint32_t oldLeftPos = 0;
    reader.batch = recycled.take();
    while (!vf.eof()) {
        AlignedCandidates cand = vf.getLineVector(opt.oneBased);
        if (cand.variants.size() == 0) continue;
        if (cand.tid != oldTid) { oldTid = cand.tid; oldLeftPos = 0; }                // DInDel.cpp:1327-1333
        if (uint32_t(cand.leftPos) < oldLeftPos) {                                    // :1335-1339
            std::cerr << "leftPos: " << uint32_t(cand.leftPos) << " oldLeftPos: " << oldLeftPos << std::endl;
            std::cerr << "Candidate variant files must be sorted on left position of window!" << std::endl;
            rc = 1;
            break;
        }
        oldLeftPos = uint32_t(cand.leftPos);
        std::vector<WindowTask> &tasks = reader.batch->tasks;                         // reused in place
        if (reader.nTasks == tasks.size()) tasks.push_back(WindowTask());
        WindowTask &T = tasks[reader.nTasks++];
        T.lines.clear();
        T.candidates = cand; T.tid = cand.tid; T.pos = uint32_t(cand.centerPos);
        T.fileLeftPos = T.leftPos = uint32_t(cand.leftPos); T.fileRightPos = T.rightPos = uint32_t(cand.rightPos);
        T.haps = NULL; T.skipped = false; T.lateSkip = false; T.passedOver = false; T.message = "ok"; T.note.clear(); T.havePairPrior = false;
        T.index = ++index;
        if (pooled) {
            Batch::Before W = { T.tid, T.fileLeftPos, T.fileRightPos, T.index };
            reader.recent.push_back(W);
        }
        // the first batches are small (an eighth, a quarter, half of --batchWindows): the GPU gets its first windows while the bulk is
        // still being prepared, and the writer its first lines
        const int want = reader.seq >= 3 ? opt.batchWindows : std::max(1, opt.batchWindows >> (3 - int(reader.seq)));
        if (int(reader.nTasks) >= want && !flush()) break;
    }
    if (reader.nTasks) flush();
    return rc;
}

int WindowLoop::run()
{
    std::vector<std::thread> prepareWorkers, computeWorkers;
    for (int pt = 0; pt < opt.prepareThreads; pt++) prepareWorkers.push_back(std::thread(&WindowLoop::prepareWorker, this, pt));
    for (int ct = 0; ct < opt.computeThreads; ct++) computeWorkers.push_back(std::thread(&WindowLoop::computeWorker, this, ct));
    std::thread writerThread(&WindowLoop::writer, this);
    int rc = 0;
    try { rc = readWindowFile(); } catch (std::string &s) { fail(s); }
    // shutdown, in this order: the batches being reduced hold views into the engines' result blocks, so the engines outlive the writer
    toPrepare.close();
    for (size_t t = 0; t < prepareWorkers.size(); t++) prepareWorkers[t].join();
    toCompute.close();
    writerThread.join();                                  // ends when every batch has come through (the last compute worker closed toReduce)
    { std::lock_guard<std::mutex> lk(done_m); reduceDone = true; }
    done_cv.notify_all();
    for (size_t t = 0; t < computeWorkers.size(); t++) computeWorkers[t].join();
    glfOutput.close();
    if (!fatal.empty()) { std::cerr << "Exception: " << fatal << std::endl; return fatalExit.load(); }
    if (rc) return rc;
    if (!opt.quiet) std::cout << "windows: " << n.windows << " skipped: " << n.skipped << " -> " << glfFile << std::endl;
    if (!opt.quiet && n.rePrepared) std::cout << "re-prepared behind late skips: " << n.rePrepared << " windows" << std::endl;
    if (opt.timing) report();
    if (opt.checkDevicePair && n.pairDisagreements.load() != 0) {            // --checkDevicePair: a certified pair that is not the host's fails the run
        std::cerr << "--checkDevicePair: " << n.pairDisagreements.load() << " certified windows whose haplotype pair the host chooses differently" << std::endl;
        return 3;
    }
    return 0;
}

void WindowLoop::report()                                 // --timing: one line; tools/n2_pipeline_bench.py and tools/pipeline_timeline.py parse it
{
    const double wall = seconds_since(t_start);
    auto sum = [](const std::vector<double> &v) { double s = 0.0; for (size_t i = 0; i < v.size(); i++) s += v[i]; return s; };
    const std::vector<std::pair<double, long> > &progress = n.progress;
    long peakKb = 0;                                                      // VmHWM of /proc/self/status
    {
        std::ifstream st("/proc/self/status");
        std::string line;
        while (std::getline(st, line)) if (line.compare(0, 6, "VmHWM:") == 0) peakKb = atol(line.c_str() + 6);
    }
    std::cout << "timing: wall=" << wall << " setup=" << t_setup << " prepare_threads=" << opt.prepareThreads << " prepare=" << sum(n.prepareOf) << " compute_threads=" << opt.computeThreads
              << " compute=" << sum(n.computeOf) << " (pack=" << sum(n.packOf) << " device=" << sum(n.deviceOf) << " unpack=" << sum(n.unpackOf) << ") reduce_threads=" << opt.reduceThreads
              << " reduce=" << n.reduce << " (work=" << n.reduceWork << " summed over the threads)" << " peak_rss_mb=" << peakKb / 1024 << " windows_per_s=" << double(n.windows) / wall;
    // the rate once the pipeline is full: from the batch that completed the first fifth of the windows to the last one
    size_t from = 0;
    while (from + 1 < progress.size() && progress[from].second * 5 < n.windows) from++;
    if (from + 1 < progress.size() && progress.back().first > progress[from].first)
        std::cout << " steady_windows_per_s=" << double(progress.back().second - progress[from].second) / (progress.back().first - progress[from].first);
    std::cout << " launches=" << n.launches.load();
    if (opt.doPooled) std::cout << " pooled=" << sum(n.pooledOf);       // of compute: the windows' sets and masks and their EM slots
    // bytes of per-base alignments / of CIGAR arrays the window loop's engines brought back; --deviceCigars: reads redone on the host
    // and the alignment bytes those windows' recomputation brought back
    std::cout << " hpos_bytes=" << n.hposBytes.load() << " cigar_bytes=" << n.cigarBytes.load() << " cigar_host_fallbacks=" << n.cigarFallbacks.load()
              << " fallback_hpos_bytes=" << n.fallbackHposBytes.load();
    if (opt.deviceRealign || opt.deviceRealignDiploid) std::cout << " realign_bytes=" << n.realignBytes.load();
    if (opt.deviceRealignDiploid) std::cout << " pair_uncertified=" << n.pairUncertified.load() << " pair_fallback_reads=" << n.pairFallbackReads.load();
    if (opt.checkDevicePair) std::cout << " pair_disagreements=" << n.pairDisagreements.load();
    // --deviceIndelKeys: bytes of key counts brought back, and pairs over 64 keys whose window was recomputed with alignments
    if (opt.deviceIndelKeys) std::cout << " indel_key_bytes=" << n.indelKeyBytes.load() << " indel_key_fallbacks=" << LikelihoodEngine::indelKeyFallbacks();
    if (opt.audit > 0) std::cout << " audit_windows=" << n.auditWindows.load() << " audit_pairs=" << n.auditPairs.load() << " audit_mismatches=" << n.auditMismatches.load();
    // when the first batch and the first 1 / 5 / 20 / 50 / 100 % of the windows were written (seconds since start)
    std::cout << " engines_ready_at=";
    for (size_t i = 0; i < n.readyAt.size(); i++) std::cout << (i ? "," : "") << n.readyAt[i];
    std::cout << " written_at=";
    size_t at = 0;
    if (!progress.empty()) std::cout << progress[0].first << "(first)";
    for (int pc : {1, 5, 20, 50, 100}) {
        while (at + 1 < progress.size() && progress[at].second * 100 < n.windows * pc) at++;
        if (!progress.empty()) std::cout << "/" << progress[at].first;
    }
    std::cout << std::endl;
}
}

// --discover: the stage in front of the loop (host/discover.hpp); throws std::string
static void runDiscovery(Options &o)
{
    const TimePoint t0 = now();
    DiscoverOptions &d = o.disc;
    if (d.vcfCandidatesOnly) d.bamFiles.clear();
    else if (o.bamPaths.empty()) d.bamFiles = readBamList(o.bamList);
    else d.bamFiles = o.bamPaths;
    CandidateStats stats;
    const long lines = discoverWindows(d, stats);
    if (!o.quiet)
        std::cout << "discovery: " << stats.candidates << " candidates in " << stats.batches << " launches (" << stats.dropped << " dropped, " << stats.overflowed
                  << " redone on the host) -> " << lines << " window lines in " << d.windowsFile() << std::endl;
    if (o.timing) std::cout << "discovery_seconds: " << seconds_since(t0) << std::endl;
}

int main(int argc, char **argv)
{
    Options options;
    int exitCode = 0;
    if (!parseOptions(argc, argv, options, exitCode)) return exitCode;
    try {
        if (options.discover) runDiscovery(options);
        int rc = 0;
        long long auditMismatches = 0;
        {
            WindowLoop loop(options);
            rc = loop.run();
            options.bamPaths = loop.bamPaths();
            auditMismatches = loop.auditMismatches();
        }
        if (rc == 0 && !options.vcfFile.empty())
            mergeOutputFiles(std::vector<std::string>(1, options.outputPrefix + ".glf.txt"), options.sampleID, options.vcfRef, 10, options.vcfFile, 20);
        if (rc == 0 && !options.pooledVcfFile.empty()) {                 // dindel_pooled2vcf, then dindel_pooled2glf, on the one file just written
            const std::vector<std::string> glf(1, options.outputPrefix + ".glf.txt");
            std::ostringstream notes;                                    // (the scripts' progress lines)
            options.pooledVcf.numBamFiles = int(options.bamPaths.size());
            pooledGlfToVcf(glf, options.pooledVcf, std::cerr, options.quiet ? static_cast<std::ostream &>(notes) : std::cout);
            if (!options.pooledGlfFile.empty())
                pooledCallsToGlf(glf, options.pooledVcfFile, options.pooledGlfFile, options.bamPaths, std::cerr, options.quiet ? static_cast<std::ostream &>(notes) : std::cout);
        }
        if (rc == 0 && auditMismatches > 0) {
            std::cerr << "audit: " << auditMismatches << " difference(s) between "
                      << (options.auditFaster ? "the --faster kernels and the shadow kernel" : "the main kernels and the long-window kernel")
                      << " on the audited windows; the output files were written" << std::endl;
            return 3;
        }
        return rc;
    } catch (std::string &s) {
        std::cerr << "Exception: " << s << std::endl;
        return 1;
    }
}
