// mm_values_load.h — the bounds-checked sequence loads of the one-launch value kernels (mm_values_reads.hip,
// mm_values_batch.hip, mm_values_text.hip): the dwords that hold a k-mer, out of a PackedView (mm_launch.h).  Whole dwords inside the view come
// from plain global loads; anything else takes the edge path, which reads single bytes inside the view and zeros outside.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mm_launch.h"

namespace mm {

// dword q of the buffer by the edge rules: whole dwords inside come from one load, others byte by byte
__host__ __device__ __forceinline__ uint32_t edge_dword(const PackedView &v, unsigned long long q) {
    if (q >= v.q_lo && q < v.q_hi) return v.d[q];
    if (q > v.q_hi) return 0u;  // (q_hi may be the partial last dword; nothing lies past it.  Also keeps 4 * q from wrapping.)
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(v.d);
    uint32_t r = 0;
    for (uint32_t b = 0; b < 4u; ++b) {
        const unsigned long long at = 4ull * q + b;
        if (at >= v.byte_lo && at < v.byte_hi) r |= (uint32_t)bytes[at] << (8u * b);
    }
    return r;
}

// whether the N dwords from dword q on lie wholly inside the view
template <int N>
__host__ __device__ __forceinline__ bool dwords_inside(const PackedView &v, unsigned long long q) {
    return q >= v.q_lo && q < v.q_hi && v.q_hi - q >= (unsigned long long)N;
}

// the N dwords from dword q on
template <int N>
__host__ __device__ __forceinline__ void load_dwords(const PackedView &v, unsigned long long q, uint32_t (&w)[N]) {
    if (dwords_inside<N>(v, q)) {
#pragma unroll
        for (int t = 0; t < N; ++t) w[t] = v.d[q + t];
    } else {  // (rare: kept rolled, the hot path above is what the registers are for)
#pragma nounroll
        for (int t = 0; t < N; ++t) w[t] = edge_dword(v, q + (unsigned long long)t);
    }
}

}  // namespace mm
