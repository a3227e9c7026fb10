// cigar_kernel.hip — getCIGAR on the device: the CIGAR of every (haplotype, read) pair from the hpos the likelihood kernels left in HBM,
// so that a realigned BAM needs a handful of (op, len) words per read instead of the read's whole per-base alignment.
//
// The specification is host/cigar.cpp (DetInDel::getCIGAR, reference DInDel.cpp:728-882), quirks included: every read base gets its
// position on the reference through the haplotype (onRef[b] = hap_ref_pos[hpos[b]], or the negative code itself), bases in front of the
// first and behind the last base with a position are soft-clipped, and the bases between them go through the reference's if-chain over the
// neighbouring pairs (onRef[b-1], onRef[b]) with the running state (op, len, anchor).
//
// One wavefront per pair, 64 read bases at a time.  A lane classifies the step INTO its base into the branch the if-chain would take:
//     GOES_ON     INS -> INS            len++ (needs op == I, else "Error(1)!")
//     CONSEC      x -> x+1              len++ (needs op == M, else "Error(3)!")
//     REF_TO_INS  x>=0 -> INS           event ("Error(2)!" unless op == M)
//     IMPOSSIBLE  other code -> INS     event ("How is this possible? (1)")
//     DEL         x -> x+d, d > 1       event ("Error(4)!" unless op == M)
//     INS_TO_REF  INS -> anchor+1       event
//     INS_DEL     INS -> anchor+d, d>1  event
//     NONE        anything else         nothing (the if-chain has no final else)
// Only the two INS -> reference branches look at `anchor`.  A base that is INS inside the aligned stretch was entered from a base with a
// position (REF_TO_INS, which sets anchor to that position) or from another INS (GOES_ON, which leaves it), or the walk has already
// thrown; so whenever those branches are reached the anchor is the value at the nearest earlier base that is not INS, which a lane finds
// with one ballot and one cross-lane read.  With that the classes depend on the data alone.  The two quiet classes are counted per
// stretch between events with popcounts of their ballots (op is constant there, so its precondition is checked once per stretch), and
// only the events — typically none to three per read — are replayed one by one, in order, on wave-uniform state.  The first failing
// precondition ends the pair with the code of the string the host throws.
//
// No floating point; the operations are written by lane 0 with ordinary vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cigar_kernel.h"
#include "cigar_walk.h"

namespace ddc {

__global__ void __launch_bounds__(64 * DD_CIGAR_WAVES) dd_cigar_kernel(CigarArgs P)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * DD_CIGAR_WAVES;
    const int64_t pair_end = P.pair_end >= 0 ? P.pair_end : P.win_pair_off[P.n_windows];
    for (int64_t pair = P.pair_begin + (int64_t)blockIdx.x * DD_CIGAR_WAVES + wave; pair < pair_end; pair += stride) {
        cigar_walk(P, pair, P.out, pair, lane);
    }
}

hipError_t launch_cigars(const CigarArgs &A, hipStream_t st)
{
    const int64_t n = A.max_pairs;
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + DD_CIGAR_WAVES - 1) / DD_CIGAR_WAVES;
    if (blocks > DD_CIGAR_MAX_BLOCKS) blocks = DD_CIGAR_MAX_BLOCKS;
    hipLaunchKernelGGL(dd_cigar_kernel, dim3((unsigned)blocks), dim3(64 * DD_CIGAR_WAVES), 0, st, A);
    return hipGetLastError();
}

} // namespace ddc
