// mm_values.h — the arithmetic of Output::values_u64 / values_u128 (src/lib.rs:584-629), shared by the single-sequence
// kernels (mm_aux.hip) and the reads kernels (mm_values_reads.hip): from the dwords that hold a k-mer to its value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

// packed-seq read_kmer: base j of the k-mer at bits 2j; read_revcomp_kmer: reversed, code ^ 2.
// w0..w2: the three dwords from the one that holds the k-mer's first base on, sh = 2 * (first base % 16).
__device__ __forceinline__ unsigned long long value_of(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t sh, uint32_t len,
                                                       int canonical, unsigned long long mask) {
    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh), hi = __builtin_amdgcn_alignbit(w2, w1, sh);
    unsigned long long v = (((unsigned long long)hi << 32) | lo) & mask;
    if (canonical) {
        unsigned long long r = __brevll(v);  // reverses bit order: pairs reversed and bit-swapped
        r = ((r & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((r & 0x5555555555555555ull) << 1);
        r >>= (64u - 2u * len);
        r ^= 0xAAAAAAAAAAAAAAAAull & mask;  // complement: code ^ 2
        v = r < v ? r : v;
    }
    return v;
}

// Output::values_u128 (src/lib.rs:587-629): up to 64 bases per value.  w[0..4]: the five dwords from the one that holds
// the first base on (zero-extended), sh as above; the value comes back as {lo, hi}.
__device__ __forceinline__ void value128_of(const unsigned long long (&w)[5], uint32_t sh, uint32_t len, int canonical,
                                            unsigned long long &lo, unsigned long long &hi) {
    unsigned long long a = w[0] | (w[1] << 32), b = w[2] | (w[3] << 32);
    lo = sh ? (a >> sh) | (b << (64u - sh)) : a;
    hi = sh ? (b >> sh) | (w[4] << (64u - sh)) : b;
    const uint32_t bits = 2u * len;  // 2 .. 128
    if (bits <= 64) {
        hi = 0;
        if (bits < 64) lo &= (1ull << bits) - 1ull;
    } else if (bits < 128) {
        hi &= (1ull << (bits - 64u)) - 1ull;
    }
    if (canonical) {
        // reverse the 2-bit groups of the 128-bit value, align to bit 0, complement (code ^ 2)
        auto revpairs = [](unsigned long long x) {
            x = __brevll(x);
            return ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((x & 0x5555555555555555ull) << 1);
        };
        unsigned long long rhi = revpairs(lo), rlo = revpairs(hi);  // 128-bit reversal
        const uint32_t s = 128u - bits;                              // shift right by s (0 .. 126)
        unsigned long long clo, chi;
        if (s == 0) { clo = rlo; chi = rhi; }
        else if (s < 64) { clo = (rlo >> s) | (rhi << (64u - s)); chi = rhi >> s; }
        else if (s == 64) { clo = rhi; chi = 0; }
        else { clo = rhi >> (s - 64u); chi = 0; }
        unsigned long long mlo = bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
        unsigned long long mhi = bits <= 64 ? 0ull : (bits >= 128 ? ~0ull : (1ull << (bits - 64u)) - 1ull);
        clo ^= 0xAAAAAAAAAAAAAAAAull & mlo;
        chi ^= 0xAAAAAAAAAAAAAAAAull & mhi;
        if (chi < hi || (chi == hi && clo < lo)) { lo = clo; hi = chi; }
    }
}

}  // namespace mm
