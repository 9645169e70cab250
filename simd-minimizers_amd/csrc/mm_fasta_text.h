// mm_fasta_text.h - the per-thread step of fasta2_text_kernel (mm_fasta2.hip): the bytes of a 32-byte piece of text that a
// 32-bit mask selects (bit i = byte i), moved together in front, as they are - no case folding, no mapping.  The rule is
// the packer's (fasta2_pack_kernel): a thread's sequence bytes are ONE run (a piece of one sequence line) or TWO (a line
// end inside the 32 bytes), each moved by one shift of the 256-bit value; any other mask (lines shorter than the piece,
// '\r' inside a line) takes the rare path.  Everything works on eight dwords with constant indices: a byte loop with a
// running output index would index registers dynamically and spill to scratch, so a shift by a variable number of bytes
// is a barrel shifter (by 16, 8, 4 bytes as dword moves, by 0..3 bytes as v_alignbyte) and the rare path is the
// compress network of Hacker's Delight 7-4 with bytes where the book moves bits (five steps: every kept byte moves
// down by the number of dropped bytes below it, one binary digit of that number per step).
// __host__ __device__: the CPU suite runs the same function through mm_debug_compact32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MM_FT_HD __host__ __device__ __forceinline__
#else
#define MM_FT_HD inline
#endif

namespace mm {

struct Compact32 {
    uint32_t d[8];   // the kept bytes in text order from byte 0 on, zeros behind them
    uint32_t count;  // how many
};

// ({hi, lo} >> 8 * sh) & 0xffffffff, sh = 0..3
MM_FT_HD uint32_t ft_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return sh ? (lo >> (8u * sh)) | (hi << (32u - 8u * sh)) : lo;
#endif
}
MM_FT_HD uint32_t ft_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }  // x != 0

// y = x >> f bytes (towards byte 0; zeros come in at the top), f = 0..31
MM_FT_HD void ft_shr_bytes(const uint32_t (&x)[8], uint32_t f, uint32_t (&y)[8]) {
    uint32_t a[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = x[i];
    a[8] = 0u;
#pragma unroll
    for (int s = 4; s >= 1; s >>= 1) {  // dword moves by 4, 2, 1
        const bool on = (f & (4u * (uint32_t)s)) != 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = on ? (i + s < 8 ? a[i + s] : 0u) : a[i];
    }
    const uint32_t b = f & 3u;
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = ft_alignbyte(a[i + 1], a[i], b);
}

// dword i of the 32-byte mask that keeps bytes [0, l), l = 0..32
MM_FT_HD uint32_t ft_low_bytes(uint32_t l, int i) {
    const int r = (int)l - 4 * i;
    return r <= 0 ? 0u : (r >= 4 ? 0xffffffffu : ((1u << (8 * r)) - 1u));
}
// a 4-bit mask (bit j = byte j) as 0xff per byte
MM_FT_HD uint32_t ft_spread4(uint32_t m4) { return (((m4 & 0xfu) * 0x00204081u) & 0x01010101u) * 0xffu; }
// inclusive prefix XOR of a 32-bit mask (bit i = XOR of bits 0..i)
MM_FT_HD uint32_t ft_pxor32(uint32_t x) {
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    return x;
}

MM_FT_HD Compact32 compact32(const uint32_t (&x)[8], uint32_t mask) {
    Compact32 r;
    r.count = (uint32_t)__builtin_popcount(mask);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.d[i] = 0u;
    if (mask == 0u) return r;
    // the first run: bytes [f1, f1 + l1)
    const uint32_t f1 = ft_ctz(mask), t1 = mask >> f1, l1 = t1 == 0xffffffffu ? 32u : ft_ctz(~t1);
    const uint32_t rest = l1 + f1 >= 32u ? 0u : (mask >> (f1 + l1)) << (f1 + l1);
    uint32_t y[8];
    ft_shr_bytes(x, f1, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.d[i] = y[i] & ft_low_bytes(l1, i);
    if (rest == 0u) return r;
    const uint32_t f2 = ft_ctz(rest), t2 = rest >> f2, l2 = t2 == 0xffffffffu ? 32u : ft_ctz(~t2);
    const uint32_t rest2 = l2 + f2 >= 32u ? 0u : (rest >> (f2 + l2)) << (f2 + l2);
    if (rest2 == 0u) {
        // the second run: bytes [f2, f2 + l2) go to [l1, l1 + l2) - a shift towards byte 0 again, f2 > l1
        ft_shr_bytes(x, f2 - l1, y);
#pragma unroll
        for (int i = 0; i < 8; ++i) r.d[i] |= y[i] & ft_low_bytes(l1 + l2, i) & ~ft_low_bytes(l1, i);
        return r;
    }
    // any mask: five steps, step j moves the bytes whose count of dropped bytes below has bit j set by 2^j bytes
    uint32_t v[8], m = mask, mk = ~mask << 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x[i] & ft_spread4(mask >> (4 * i));  // (dropped bytes leave as zeros)
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint32_t mp = ft_pxor32(mk), mv = mp & m;
        m = (m ^ mv) | (mv >> (1u << j));
        uint32_t t[8], ts[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            t[i] = v[i] & ft_spread4(mv >> (4 * i));
            v[i] ^= t[i];
        }
        ft_shr_bytes(t, 1u << j, ts);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] |= ts[i];
        mk &= ~mp;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) r.d[i] = v[i];
    return r;
}

}  // namespace mm
