// mm_values.h — the arithmetic of Output::values_u64 / values_u128 (src/lib.rs:584-629), shared by the single-sequence
// kernels (mm_aux.hip), the reads and batch kernels (mm_values_reads.hip, mm_values_batch.hip) and the text kernels
// (mm_values_text.hip): from the dwords that hold a k-mer to its value.  The steps behind the funnel shift - masking to
// 2 * len bits and the canonical minimum - are __host__ __device__ (mm_debug_values_text runs them on the host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

// the 2-bit groups of a 64-bit word in reverse order (bit order reversed, then the bits of every pair swapped back)
__host__ __device__ __forceinline__ unsigned long long reverse_pairs(unsigned long long x) {
    x = __builtin_bitreverse64(x);
    return ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((x & 0x5555555555555555ull) << 1);
}

// packed-seq read_revcomp_kmer against read_kmer: min(v, reversed and complemented v); v holds len <= 32 bases and
// nothing above them, mask = the low 2 * len bits.
__host__ __device__ __forceinline__ unsigned long long canonical_value(unsigned long long v, uint32_t len,
                                                                      unsigned long long mask) {
    unsigned long long r = reverse_pairs(v);
    r >>= (64u - 2u * len);
    r ^= 0xAAAAAAAAAAAAAAAAull & mask;  // complement: code ^ 2
    return r < v ? r : v;
}

// The tail of a 128-bit value: {lo, hi} holds the bases from bit 0 on and anything above them; keeps 2 * len bits
// (len 1 .. 64) and takes the canonical minimum.
__host__ __device__ __forceinline__ void finish_value128(uint32_t len, int canonical, unsigned long long &lo,
                                                         unsigned long long &hi) {
    const uint32_t bits = 2u * len;  // 2 .. 128
    // (masks by value, not stores under branches: lo and hi stay in registers wherever this is inlined)
    const unsigned long long mlo = bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
    const unsigned long long mhi = bits <= 64 ? 0ull : (bits >= 128 ? ~0ull : (1ull << (bits - 64u)) - 1ull);
    lo &= mlo;
    hi &= mhi;
    if (canonical) {
        // reverse the 2-bit groups of the 128-bit value, align to bit 0, complement (code ^ 2)
        unsigned long long rhi = reverse_pairs(lo), rlo = reverse_pairs(hi);  // 128-bit reversal
        const uint32_t s = 128u - bits;                                        // shift right by s (0 .. 126)
        unsigned long long clo, chi;
        if (s == 0) { clo = rlo; chi = rhi; }
        else if (s < 64) { clo = (rlo >> s) | (rhi << (64u - s)); chi = rhi >> s; }
        else if (s == 64) { clo = rhi; chi = 0; }
        else { clo = rhi >> (s - 64u); chi = 0; }
        clo ^= 0xAAAAAAAAAAAAAAAAull & mlo;
        chi ^= 0xAAAAAAAAAAAAAAAAull & mhi;
        if (chi < hi || (chi == hi && clo < lo)) { lo = clo; hi = chi; }
    }
}

// packed-seq read_kmer: base j of the k-mer at bits 2j; read_revcomp_kmer: reversed, code ^ 2.
// w0..w2: the three dwords from the one that holds the k-mer's first base on, sh = 2 * (first base % 16).
__device__ __forceinline__ unsigned long long value_of(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t sh, uint32_t len,
                                                       int canonical, unsigned long long mask) {
    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh), hi = __builtin_amdgcn_alignbit(w2, w1, sh);
    unsigned long long v = (((unsigned long long)hi << 32) | lo) & mask;
    if (canonical) v = canonical_value(v, len, mask);
    return v;
}

// Output::values_u128 (src/lib.rs:587-629): up to 64 bases per value.  w[0..4]: the five dwords from the one that holds
// the first base on (zero-extended), sh as above; the value comes back as {lo, hi}.
__device__ __forceinline__ void value128_of(const unsigned long long (&w)[5], uint32_t sh, uint32_t len, int canonical,
                                            unsigned long long &lo, unsigned long long &hi) {
    unsigned long long a = w[0] | (w[1] << 32), b = w[2] | (w[3] << 32);
    lo = sh ? (a >> sh) | (b << (64u - sh)) : a;
    hi = sh ? (b >> sh) | (w[4] << (64u - sh)) : b;
    finish_value128(len, canonical, lo, hi);
}

}  // namespace mm
