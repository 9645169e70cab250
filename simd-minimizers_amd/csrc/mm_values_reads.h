// mm_values_reads.h — which read a value belongs to (mm_values_reads.hip; mm_debug_values_read_of runs the same function
// on the host).  Plain C++: a host-only program may include it without the HIP headers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MM_HOST_DEVICE __host__ __device__
#else
#define MM_HOST_DEVICE
#endif

namespace mm {

// Offsets a workgroup stages in LDS (8 bytes each): a workgroup whose values span more reads than this (runs of empty
// reads) searches the offsets in global memory instead.
constexpr uint32_t kValuesReadsStage = 2048;

// The read of value `idx`: the LARGEST r in [lo, hi] with offsets[r] <= idx, given offsets[lo] <= idx and offsets
// non-decreasing - so empty reads (offsets[r] == offsets[r + 1]) are never the answer unless they end the range.  Over
// [0, n_reads] this is searchsorted(offsets, idx, 'right') - 1.  `Offsets` is any random-access view of 64-bit offsets
// (a pointer to global memory, to LDS, or host memory).
template <class Offsets>
MM_HOST_DEVICE inline uint64_t values_read_of(Offsets offsets, uint64_t lo, uint64_t hi, uint64_t idx) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;  // (upper middle: lo < mid <= hi, so both branches shrink the range)
        if ((uint64_t)offsets[mid] <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace mm
