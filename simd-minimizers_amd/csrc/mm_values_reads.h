// mm_values_reads.h — which read a value belongs to (mm_values_reads.hip; mm_debug_values_read_of runs the same function
// on the host), and the view of a buffer that the one-launch value kernels load from.  Plain C++: a host-only program
// may include it without the HIP headers.
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

// A buffer of any byte alignment as whole dwords plus its byte range: d = the address rounded down to a dword, bytes
// [byte_lo, byte_hi) of d are the caller's, dwords [q_lo, q_hi) lie wholly inside them (none when q_lo >= q_hi); symbol
// p of the buffer is symbol base0 + p of d.
struct PackedView {
    const uint32_t *d;
    unsigned long long q_lo, q_hi;
    unsigned long long byte_lo, byte_hi;
    unsigned long long base0;
};
// q_lo and q_hi from the byte range
MM_HOST_DEVICE inline void view_whole_dwords(PackedView &v) {
    v.q_lo = v.byte_lo ? 1 : 0;
    v.q_hi = v.byte_hi >> 2;
}
// The view of `bytes` bytes at `address`, the buffer's symbol 0 being symbol `base_offset` of its first byte, at
// `per_byte` symbols a byte (4: packed bases, 1: text).
MM_HOST_DEVICE inline PackedView packed_view(uint64_t address, uint64_t bytes, uint64_t base_offset, uint32_t per_byte) {
    PackedView v;
    v.byte_lo = address & 3u;
    v.d = reinterpret_cast<const uint32_t *>(static_cast<uintptr_t>(address - v.byte_lo));
    v.byte_hi = v.byte_lo + bytes;
    v.base0 = base_offset + per_byte * v.byte_lo;
    view_whole_dwords(v);
    return v;
}

}  // namespace mm
