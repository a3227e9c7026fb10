// windows.hpp — step 3 of the workflow: candidate lines (`tid pos variant ... # count ...`, what dindel_candidates writes) -> window files
// (`tid leftPos rightPos pos,variant ...`, what dindel_gpu --varFile reads).  Restates the reference's Python-2 scripts
// python/makeWindows.py (split_and_merge, write_output_candidates) and python/selectCandidates.py rule for rule; plain C++, no GPU:
// the step is a sort and a walk over the candidates.
//
//   input lines          python/makeWindows.py:137-161   split on blanks; field 0 the target (a string), field 1 the position (an integer),
//                        fields 2... up to a `#` or the end of the line the variants; lines of one (target, position) accumulate.
//                        A target that parses as an integer > 24 or as 0 gets the warning of python/makeWindows.py:144-149 on stderr.
//   clustering           python/makeWindows.py:177-186   per target over its sorted distinct positions; see clusterKeys below.
//   cluster contents     python/makeWindows.py:189-199, python/makeWindows.py:64   the distinct (original position, variant string)
//                        pairs of the cluster's positions: duplicates collapse.
//   variant shapes       python/makeWindows.py:5-31      -SEQ deletion, refEnd = pos + len - 1; +SEQ insertion, refEnd = pos - 1; any other
//                        string of exactly four characters a SNP, refEnd = pos; anything else, or a string shorter than two characters,
//                        throws "Unrecognized variant: X".
//   window bounds        python/makeWindows.py:62-75     minRef starts at 2,000,000,000 and maxRef at 0 (so an insertion at 5 alone gives
//                        0 64 and one at 0 gives 0 60); leftPos = max(0, minRef - 60), rightPos = maxRef + 60.
//   lines                python/makeWindows.py:89-107    `tid leftPos rightPos` and up to 16 ` pos,variant` tokens; a cluster of more
//                        continues on further lines with the same bounds.  A cluster without any variant writes no line (and counts).
//   files                python/makeWindows.py:46-57, python/makeWindows.py:205-206   PREFIX.N.txt, N from 1 and running on across
//                        targets; a new file for every target, and when the counter EXCEEDS numWindowsPerFile; the counter counts
//                        clusters (not lines) and restarts at 0, so a file holds numWindowsPerFile + 2 clusters.
//   stderr               python/makeWindows.py:163-169, python/makeWindows.py:202, python/makeWindows.py:114-117   the summary lines;
//                        the mean window size is Python 2's integer (floor) division.
//   the filter           python/selectCandidates.py:6-63   see selectCandidates below.
//
// Where the scripts' order is that of a Python-2 dict or set, i.e. not defined, it is defined here:
//   targets follow their first appearance in the input (python/makeWindows.py:168, python/makeWindows.py:175 walk a dict);
//   the tokens of a cluster go by original position, then by first appearance in the input (python/makeWindows.py:64 walks a set);
//   the filter's variants within a position follow their first appearance (python/selectCandidates.py:8 walks a dict).
#ifndef DINDEL_WINDOWS_HPP
#define DINDEL_WINDOWS_HPP
#include <iosfwd>
#include <string>
#include <vector>

namespace dindel {

// The fixed point of the loop of python/makeWindows.py:180-186 in closed form: keys[p] is the first position of the run of positions
// around positions[p] in which every gap between neighbours is <= minDist (single linkage).  `positions` is sorted and distinct.
//
// The loop as written, with P = positions and N = newPosition (N starts as a copy of P), repeats until a pass changes nothing:
//     for p in 1 ... len-1:  if N[p] != N[p-1] and N[p] - P[p-1] <= minDist:  N[p] = N[p-1]
// Proof that it ends with N[p] = N[p-1] exactly when P[p] - P[p-1] <= minDist, and N[p] = P[p] otherwise:
//   (a) N[p] only ever takes values N[q] held for some q <= p, so N[p] <= P[p] throughout, and N[0] = P[0] never changes.
//   (b) While p has not been assigned, N[p] = P[p] > P[p-1] >= N[p-1] (distinct, sorted, (a)), so the first test holds and the second
//       reads P[p] - P[p-1] <= minDist: it does not depend on the state.  A p whose gap is larger is therefore never assigned and
//       keeps N[p] = P[p]; a p whose gap is small enough is assigned in the first pass.
//   (c) Once assigned, N[p] is a value N[p-1] held, hence <= P[p-1] by (a): N[p] - P[p-1] <= 0.  This is the difference that "goes
//       negative after a join".  For minDist >= 0 the second test then always holds, so whenever N[p-1] moves on (its own join),
//       N[p] != N[p-1] and the next pass sets N[p] = N[p-1] again: at the fixed point N[p] = N[p-1].  For minDist < 0 no gap (>= 1)
//       passes (b), nothing is ever assigned, and the statement holds with no joins at all.
//   (d) Every assignment strictly lowers N[p] within a finite set, so the loop ends.  By induction over p the fixed point gives every
//       position the first position of its run.
std::vector<long> clusterKeys(const std::vector<long> &positions, long minDist);

// One output file: the name's number N (PREFIX.N.txt) and its lines, without the newline
struct WindowFile {
    int number;
    std::vector<std::string> lines;
};

// split_and_merge over candidate lines (each without its newline).  Appends the files to `files`; the summary lines go to `err`, the
// `N lines read` progress of python/makeWindows.py:142-143 to `progress` if it is not NULL.  Throws std::string ("Unrecognized
// variant: X", and in place of Python's IndexError / ValueError on a line without two fields or with a position that is no integer).
void makeWindows(const std::vector<std::string> &lines, long minDist, long numWindowsPerFile, std::vector<WindowFile> &files, std::ostream &err,
                 std::ostream *progress = NULL);

// selectCandidates of python/selectCandidates.py:14-66 with emptyBuffer (python/selectCandidates.py:6-10): consecutive lines of one
// position are merged, the counts behind `#` summed per variant string, and one `chr pos var # count` line is returned per variant
// with minCount <= count <= maxCount.  Throws the script's two errors (a target that comes back; a position that goes down) as
// std::string.  As in the script the buffer is NOT emptied when the target changes (python/selectCandidates.py:35-41 set currPos
// to -1, so python/selectCandidates.py:52 skips the call): the last position of every target but the last one is left out.
// "Analyzing chromosome X" goes to `err`.
std::vector<std::string> selectCandidates(const std::vector<std::string> &lines, long minCount, long maxCount, std::ostream &err);

struct WindowOptions {
    std::string inputVarFile, windowFilePrefix;       // -i, -w
    std::string oneFile;                              // --oneFile F: every line goes to F instead of PREFIX.N.txt
    std::string selectedFile;                         // --selectedFile F: what the filter kept
    long minDist, numWindowsPerFile;                  // -m (20), -n (1000)
    bool filter; long minCount, maxCount;             // --minCount / --maxCount: either one switches the filter on (defaults 2 / 10000000)
    bool quiet;                                       // no summary on stderr, no progress on stdout (errors are still thrown)
    WindowOptions() : minDist(20), numWindowsPerFile(1000), filter(false), minCount(2), maxCount(10000000), quiet(false) {}
};
// reads the input file, filters, clusters and writes the files; returns the number of window lines written.  Throws std::string.
long writeWindows(const WindowOptions &opt, std::ostream &err);

// the tool (host/dindel_windows.cpp is this call): the reference's options, messages and exit codes (python/makeWindows.py:209-227)
int windowsMain(int argc, char **argv);

} // namespace dindel
#endif
