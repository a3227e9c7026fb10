// faster_model.h — the "--faster" model (ObservationModelS, reference Faster.cpp) as device code shared by its two kernels:
// dd_faster_kernel (faster_kernel.hip: everything of a pair in LDS) and dd_faster_long_kernel (faster_long_kernel.hip: back-pointers,
// vote histogram and state path in an HBM tile).  Each piece of the model is written once:
//   faster_model.h (this file)   the small helpers: map_char, wave_sync, gmax4, bmid, FOLD, FAST_EPS, FNEG_INF;
//   faster_sstate.inc            SStateHMM: emissions, the two sweeps towards bMid, the join at bMid;
//   faster_pair_end.inc          firstBase / lastBase, var_covered, the filterHaplotypes coverage test, the final store.
// The two .inc files are fragments of a kernel body, included at the one place of each kernel where the text used to stand, and use the
// kernel's locals by name (each lists them at its top); where the pointers lead (LDS or HBM) is the kernel's business.  They are not
// functions because the function forms that were tried (a struct of pointers, plain parameters, force-inlined or not, lambdas kept inside)
// all changed dd_faster_kernel's register allocation (scratch 76 -> 64..88 bytes, up to 800 more instructions): the 16-source loops sit
// at the 256-VGPR limit.  As fragments both kernels compile to the same machine code as before, instruction for instruction.
// What differs for real stays in the kernels: work distribution, read staging, the vote histogram and top-15 selection, backtrack, mapState.
#ifndef DD_FASTER_MODEL_H
#define DD_FASTER_MODEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>   // the fragments' std::integral_constant
#include "hmm_kernel.h"

namespace ddfm {

#define FAST_EPS 1e-7
#define FNEG_INF (-__builtin_huge_val())

__device__ __forceinline__ int map_char(unsigned c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 0; }

// LDS traffic between lanes of one wavefront: DS operations of a wave execute in order; this only pins the compiler.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// wave-uniform maximum of a value that is uniform inside each 16-lane group
__device__ __forceinline__ int gmax4(int v)
{
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    const int ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// bMid — ObservationModelS::computeBMid (Faster.cpp:60-88)
__device__ __forceinline__ int bmid(uint32_t hapStart, int hlen, uint32_t mReadStart, int L)
{
    const uint32_t hapEnd = hapStart + (uint32_t)hlen;
    const uint32_t readEnd = mReadStart + (uint32_t)L - 1u;
    int bMid;
    if (mReadStart > hapEnd) bMid = 0;
    else if (readEnd < hapStart) bMid = L - 1;
    else {
        const uint32_t olStart = (hapStart > mReadStart) ? hapStart : mReadStart;
        const uint32_t olEnd = (hapEnd > readEnd) ? readEnd : hapEnd;
        bMid = ((int)olEnd - (int)olStart) / 2 + (int)olStart - (int)mReadStart;
    }
    if (bMid < 0) bMid = 0;
    if (bMid >= L) bMid = L - 1;
    return bMid;
}

// `if (nv > cur + EPS) { cur = nv; bp = code; }` (Faster.cpp:383 and every other update of the model)
#define FOLD(cur, bp, nvv, code, ok)                         \
    do {                                                     \
        const double nv__ = (nvv);                           \
        const bool t__ = (ok) && nv__ > (cur) + FAST_EPS;    \
        (cur) = t__ ? nv__ : (cur);                          \
        (bp) = t__ ? (code) : (bp);                          \
    } while (0)

} // namespace ddfm
#endif
