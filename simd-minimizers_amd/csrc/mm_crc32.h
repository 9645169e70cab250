// mm_crc32.h - the gzip CRC32 (RFC 1952) written once for host and device: the verify kernel (mm_crc32.hip, one workgroup
// per BGZF block), the host entries (mm_debug_crc32, the stream's host-inflated blocks) and the stand-alone check program
// (tests/cxx/crc32_check.cpp) all run this code.  Plain C++, no HIP header needed.  The reference reads compressed files
// through its loader's decompressor on the CPU (needletail::parse_fastx_file, bench/src/lib.rs:51-82), which checks every
// member's CRC32; it has no other counterpart.
//
// The code: reflected polynomial 0xEDB88320, initial value 0xFFFFFFFF, final complement.  A register value is a polynomial
// over GF(2) modulo P with bit 31 = x^0 and bit 0 = x^31; one zero BIT through the register multiplies it by x.
//   L(m)        the pure linear register over the bytes m: initial value 0, no complement
//   crc32(m)  = ~(0xFFFFFFFF * x^(8 |m|)  xor  L(m)): starting the register of the FIRST segment at 0xFFFFFFFF folds the
//               initial value in once, the complement is taken once at the end
//   L(A || B) = L(A) * x^(8 |B|) mod P  xor  L(B): segments are computed independently and combined (crc32_combine)
// Slicing-by-4: table k (k = 0..3) holds L(byte i followed by k zero bytes), so four bytes cost four look-ups and one step.
// Words are read little-endian (x86-64 and gfx950 both are).
//
// The segment plan (crc32_plan) is the kernel's: a block of `isize` bytes that begins `lo` bytes behind a 16-byte boundary is
// cut at multiples of S bytes counted from that boundary, S a multiple of 16, into T <= 256 segments: segment t covers
// [max(t S, lo), min((t + 1) S, lo + isize)), so only segment 0 has an unaligned front and only segment T - 1 a short end
// of r = lo + isize - (T - 1) S bytes.  With u = T - 2 - t the distance from the last but one segment,
//   L(block) = x^(8 r) * sum_u L(segment T - 2 - u) * (x^(8 S))^u  xor  L(segment T - 1)
// and the sum is a tree over u in which every pair of one level takes the same multiplier (x^(8 S), squared per level) and
// absent segments are zeros; the short last segment needs the one shift of its own.  crc32_plan_combine runs that tree on
// the host, step for step as the kernel's threads do.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MM_CRC32_HD __host__ __device__ __forceinline__
#else
#define MM_CRC32_HD inline
#endif

namespace mm {

constexpr uint32_t kCrc32Poly = 0xEDB88320u;
constexpr uint32_t kCrc32One = 0x80000000u;  // x^0
constexpr uint32_t kCrc32Threads = 256;      // segments of the plan at most (the kernel's workgroup)

// c * x mod P: one zero bit through the register
MM_CRC32_HD constexpr uint32_t crc32_mulx(uint32_t c) { return (c >> 1) ^ (kCrc32Poly & (0u - (c & 1u))); }

// entry i of slicing table k: L(byte i followed by k zero bytes)
MM_CRC32_HD constexpr uint32_t crc32_table_entry(uint32_t k, uint32_t i) {
    uint32_t c = i;
    for (uint32_t s = 0; s < 8 * (k + 1); ++s) c = crc32_mulx(c);
    return c;
}

// a * b mod P in 32 shift/xor steps, the same for every a and b (no data-dependent branch: lanes stay together)
MM_CRC32_HD constexpr uint32_t crc32_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = crc32_mulx(b);
    }
    return p;
}

struct Crc32Pow8 {  // v[j] = x^(8 * 2^j)
    uint32_t v[32];
    constexpr Crc32Pow8() : v{} {
        uint32_t p = 0x00800000u;  // x^8
        for (uint32_t j = 0; j < 32; ++j) {
            v[j] = p;
            p = crc32_mulmod(p, p);
        }
    }
};

// x^(8 n) mod P by square-and-multiply: what n zero BYTES multiply the register by.  (x has an order that divides
// 2^32 - 1, so x^(8 * 2^32) = x^8 and the table wraps.)
MM_CRC32_HD constexpr uint32_t crc32_xpow8(uint64_t n) {
    constexpr Crc32Pow8 k{};
    uint32_t p = kCrc32One;
    for (uint32_t j = 0; n; n >>= 1, ++j)
        if (n & 1u) p = crc32_mulmod(p, k.v[j & 31u]);
    return p;
}

// the register after n_bytes zero bytes
MM_CRC32_HD constexpr uint32_t crc32_shift(uint32_t c, uint64_t n_bytes) { return crc32_mulmod(c, crc32_xpow8(n_bytes)); }

// L(A || B) from L(A), L(B) and |B|; with la / lb two finished gzip CRC32s it is the CRC32 of A || B as well (the initial
// values and complements cancel, as in zlib's crc32_combine)
MM_CRC32_HD constexpr uint32_t crc32_combine(uint32_t la, uint32_t lb, uint64_t b_bytes) { return crc32_shift(la, b_bytes) ^ lb; }

// one byte / one little-endian word through the register; t = the four slicing tables back to back (1024 words)
MM_CRC32_HD uint32_t crc32_step_byte(const uint32_t *t, uint32_t c, uint32_t b) { return t[(c ^ b) & 255u] ^ (c >> 8); }
MM_CRC32_HD uint32_t crc32_step_word(const uint32_t *t, uint32_t c, uint32_t w) {
    c ^= w;
    return t[768u + (c & 255u)] ^ t[512u + ((c >> 8) & 255u)] ^ t[256u + ((c >> 16) & 255u)] ^ t[c >> 24];
}

struct Crc32Plan {
    uint32_t S;  // bytes per segment, a multiple of 16
    uint32_t T;  // segments that hold a byte, 1 .. 256 (0: an empty block)
    uint32_t r;  // bytes of segment T - 1 (with T == 1: lo + isize)
};
// lo < 16, isize <= 65536
MM_CRC32_HD constexpr Crc32Plan crc32_plan(uint32_t lo, uint32_t isize) {
    const uint32_t hi = lo + isize;
    uint32_t S = ((hi + kCrc32Threads - 1) / kCrc32Threads + 15u) & ~15u;
    if (S < 16u) S = 16u;
    const uint32_t T = isize ? (hi + S - 1) / S : 0u;
    return Crc32Plan{S, T, T ? hi - (T - 1) * S : 0u};
}

// ---- host only below

struct Crc32Tables {
    uint32_t t[1024];
    constexpr Crc32Tables() : t{} {
        for (uint32_t i = 0; i < 256; ++i) t[i] = crc32_table_entry(0, i);
        // (a zero byte behind the entry below: the same values as crc32_table_entry(k, i), in fewer steps)
        for (uint32_t k = 1; k < 4; ++k)
            for (uint32_t i = 0; i < 256; ++i) t[256 * k + i] = t[t[256 * (k - 1) + i] & 255u] ^ (t[256 * (k - 1) + i] >> 8);
    }
};
inline constexpr Crc32Tables kCrc32Tables{};

// the register c over p[0 .. n): bit by bit, byte-wise with table 0, and sliced by four
inline uint32_t crc32_linear_bitwise(uint32_t c, const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int s = 0; s < 8; ++s) c = crc32_mulx(c);
    }
    return c;
}
inline uint32_t crc32_linear_bytewise(uint32_t c, const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; ++i) c = crc32_step_byte(kCrc32Tables.t, c, p[i]);
    return c;
}
inline uint32_t crc32_linear(uint32_t c, const uint8_t *p, size_t n) {
    size_t i = 0;
    for (; i + 4 <= n; i += 4) {
        uint32_t w;
        memcpy(&w, p + i, 4);
        c = crc32_step_word(kCrc32Tables.t, c, w);
    }
    for (; i < n; ++i) c = crc32_step_byte(kCrc32Tables.t, c, p[i]);
    return c;
}

// zlib's interface: crc = 0 for the first bytes, the value returned before for bytes that follow
inline uint32_t crc32_bytes(uint32_t crc, const uint8_t *p, size_t n) { return ~crc32_linear(~crc, p, n); }

// The kernel's combine on the host: seg[t] = the register of segment t of the plan (segment 0 started at 0xFFFFFFFF, the
// others at 0).  Returns the finished CRC32.
inline uint32_t crc32_plan_combine(const Crc32Plan &plan, const uint32_t *seg) {
    if (plan.T == 0) return 0;
    uint32_t red[kCrc32Threads] = {};
    for (uint32_t t = 0; t + 2 <= plan.T; ++t) red[plan.T - 2 - t] = seg[t];
    uint32_t m = crc32_xpow8(plan.S);
    for (uint32_t stride = 1; stride + 1 < plan.T; stride <<= 1) {
        for (uint32_t u = 0; u + stride < kCrc32Threads; u += 2 * stride) red[u] ^= crc32_mulmod(red[u + stride], m);
        m = crc32_mulmod(m, m);
    }
    const uint32_t last = seg[plan.T - 1];
    return ~(plan.T > 1 ? crc32_mulmod(red[0], crc32_xpow8(plan.r)) ^ last : last);
}

// A block of isize bytes at p, as if it began lo bytes behind a 16-byte boundary, through the plan: every segment by
// crc32_linear, then the combine.  Equal to crc32_bytes(0, p, isize) for every lo and isize.
inline uint32_t crc32_bytes_planned(const uint8_t *p, uint32_t isize, uint32_t lo) {
    const Crc32Plan plan = crc32_plan(lo, isize);
    uint32_t seg[kCrc32Threads] = {};
    for (uint32_t t = 0; t < plan.T; ++t) {
        const uint32_t beg = t ? t * plan.S : lo, end = t + 1 == plan.T ? lo + isize : (t + 1) * plan.S;
        seg[t] = crc32_linear(t ? 0u : 0xFFFFFFFFu, p + (beg - lo), end - beg);
    }
    return crc32_plan_combine(plan, seg);
}

}  // namespace mm
